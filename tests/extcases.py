"""Hand-planted inputs of the extension stage (arx_selftest_ext_stage, the restatement's ora_chain2aln, the reference's mem_chain2aln): the 60 kb
genome of three contigs of tests/postcases.py, reads of at most 250 bases, and chains and seeds written directly, in the rows ora_chains hands out.
mem_chain2aln is a pure function of its rows, the read and the index, so a seed need not be what seeding would find -- several cases use a seed that
lies off the read's true diagonal on purpose.  Legal input is what the reference's assert(c->rid == rid) and its fetches accept (oracle/arx_oracle.h).

Every case has a name, says which edge it must reach and carries a predicate over the restatement's shape rows, call list and regions that shows
the edge; where the answer follows from how the read was made it is written down too (regions per chain, whole region rows).  A case whose shape does
not show its edge fails check_edges().  The inputs were found on the CPU and are constants here, as postcases.PROBE_SEED is.

Used by tests/test_ext_cases_hostsim.py (the restatement against these expectations, the host double against the restatement),
tests/test_oracle_vs_ref.py and tests/golden/make_ext_stage_golden.py (the restatement against the reference) and tests/test_ext_stage_gpu.py."""
import numpy as np

import oradrv
from postcases import Genome, _rc

EXT_BOUNDS = (32, 48, 64, 96, 128, 160)   # arx_dev.h ext_class
SH = {n: i for i, n in enumerate(oradrv.Oracle.C2A_SHAPE_FIELDS)}
CL = {n: i for i, n in enumerate(oradrv.Oracle.C2A_CALL_FIELDS)}
RG = {n: i for i, n in enumerate(oradrv.REG_FIELDS)}
FRAC_REP_BITS = int(np.array([0.25], dtype=np.float32).view(np.uint32)[0])   # any bits: they must come back in every region


def ext_class(qlen):
    return int(np.searchsorted(EXT_BOUNDS, qlen, side="right"))


class Cases:
    """The reads of one batch.  add() takes seeds in doubled coordinates: chains = [(rid, [(rbeg, qbeg, len), ...]), ...]."""

    def __init__(self, g, name):
        self.g, self.name, self.reads = g, name, []
        self.L = int(g.off[-1])

    def at(self, ctg, p):
        return int(self.g.off[ctg]) + p

    def ref(self, ctg, s, n):
        assert 0 <= s and s + n <= len(self.g.seqs[ctg]), (ctg, s, n)
        return self.g.seqs[ctg][s:s + n].copy()

    def add(self, name, edge, read, chains, check=None, n_regs=None, regs=None, rev=False):
        """edge: what the case must reach, in words; check(sh, calls, regs) -> bool shows it from the restatement's rows; n_regs: regions per chain,
        regs: {index: (rb, re, qb, qe, score, truesc, w)} written down by hand.  rev: the same alignment read from the other strand."""
        read = np.asarray(read, dtype=np.uint8)
        assert 1 <= len(read) <= 250
        if rev:
            lq = len(read)
            read = _rc(read)
            chains = [(rid, [(2 * self.L - (rb + ln), lq - (qb + ln), ln) for rb, qb, ln in sd]) for rid, sd in chains]
            if regs:
                regs = {k: (2 * self.L - v[1], 2 * self.L - v[0], lq - v[3], lq - v[2]) + tuple(v[4:]) for k, v in regs.items()}
        self.reads.append(dict(name=name, edge=edge, read=read, chains=chains, check=check, n_regs=n_regs, regs=regs))

    def rows(self):
        """-> dict(seqs, lens, n_chain, chains, n_seed, seeds, frb, chain_read): what api.selftest_ext_stage takes; per read also r['ch'], r['sd']"""
        ch_all, sd_all, n_chain, n_seed, chain_read = [], [], [], [], []
        for ri, r in enumerate(self.reads):
            ch, sd = [], []
            for rid, seeds in r["chains"]:
                ch.append((seeds[0][0] if seeds else 0, rid, len(seeds), len(sd), sum(s[2] for s in seeds), 3, -1, 0))
                sd += [(rb, qb, ln, ln) for rb, qb, ln in seeds]
            r["ch"], r["sd"] = np.array(ch, dtype=np.int64).reshape(-1, 8), np.array(sd, dtype=np.int64).reshape(-1, 4)
            ch_all.append(r["ch"]); sd_all.append(r["sd"]); n_chain.append(len(ch)); n_seed.append(len(sd)); chain_read += [ri] * len(ch)
        return dict(seqs=np.concatenate([r["read"] for r in self.reads]), lens=np.array([len(r["read"]) for r in self.reads], dtype=np.int32),
                    n_chain=np.array(n_chain, dtype=np.int32), chains=np.concatenate(ch_all), n_seed=np.array(n_seed, dtype=np.int32), seeds=np.concatenate(sd_all),
                    frb=np.full(len(self.reads), FRAC_REP_BITS, dtype=np.uint32), chain_read=np.array(chain_read, dtype=np.int64))


def _sub(read, *pos):
    read = read.copy()
    for p in pos:
        read[p] = (read[p] + 1) & 3
    return read


def _calls_of(calls, chain, side=None):
    m = calls[:, CL["chain"]] == chain
    if side is not None:
        m &= calls[:, CL["side"]] == side
    return calls[m]


def build_main(g):
    """The named cases, one read each."""
    c = Cases(g, "main")
    rng = np.random.default_rng(20241020)
    at, ref = c.at, c.ref
    whole = lambda s, n, sc=None, w=100: (s, s + n, 0, n, n if sc is None else sc, n if sc is None else sc, w)   # noqa: E731
    # ---- a read with no chains first (and one in the middle and one last, below)
    c.add("no chains, first read", "n_chain == 0 at read 0", ref(0, 100, 150), [], check=lambda sh, ca, rg: len(sh) == 0 and len(rg) == 0, n_regs=[])
    # ---- dependencies
    s = at(0, 1000)
    c.add("two independent chains", "windows do not touch: no dependency, regions in chain order", ref(0, 1000, 150),
          [(0, [(s + 40, 40, 30)]), (1, [(at(1, 2000) + 60, 60, 25)])],
          check=lambda sh, ca, rg: sh[0, SH["n_dep"]] == 0 and sh[1, SH["n_dep"]] == 0 and sh[0, SH["rmax1"]] < sh[1, SH["rmax0"]] and rg[0, RG["rid"]] == 0 and rg[1, RG["rid"]] == 1,
          n_regs=[1, 1], regs={0: whole(s, 150)})
    c.add("explained later chain", "a seed inside the earlier window that the earlier region explains: 0 regions, and only if it waited", ref(0, 1000, 150),
          [(0, [(s + 40, 40, 30)]), (0, [(s + 90, 90, 25)])],
          check=lambda sh, ca, rg: sh[1, SH["n_dep"]] == 1 and sh[1, SH["skipped"]] == 1 and sh[1, SH["regs"]] == 0 and len(_calls_of(ca, 1)) == 0,
          n_regs=[1, 0], regs={0: whole(s, 150)})
    c.add("off-diagonal later chain", "the same, but the seed lies off the diagonal by more than the band: waits, then extends", ref(0, 1000, 150),
          [(0, [(s + 40, 40, 30)]), (0, [(s + 10, 90, 25)])],
          check=lambda sh, ca, rg, s=s: sh[1, SH["n_dep"]] == 1 and sh[1, SH["skipped"]] == 0 and sh[1, SH["regs"]] == 1 and rg[0, RG["rb"]] <= s + 10 and s + 35 <= rg[0, RG["re"]]
          and len(_calls_of(ca, 1)) == 2,
          n_regs=[1, 1], regs={0: whole(s, 150)})
    c.add("three deep", "c3 waits for c2, which waits for c1; c3 is clear of c1", ref(0, 1000, 150),
          [(0, [(s + 40, 40, 30)]), (0, [(s + 100, 20, 20), (s + 400, 100, 20)]), (0, [(s + 440, 60, 20)])],
          check=lambda sh, ca, rg, s=s: sh[1, SH["dep_last"]] == 0 and sh[2, SH["n_dep"]] == 1 and sh[2, SH["dep_last"]] == 1 and s + 440 > sh[0, SH["rmax1"]],
          n_regs=None)
    c.add("straddles rmax1", "no seed fully inside the earlier window, one straddling its end: independent", ref(0, 1000, 150),
          [(0, [(s + 40, 40, 30)]), (0, [(s + 215, 100, 25)])],
          check=lambda sh, ca, rg, s=s: sh[1, SH["n_dep"]] == 0 and s + 215 < sh[0, SH["rmax1"]] < s + 240, n_regs=[1, 1], regs={0: whole(s, 150)})
    c.add("empty chains", "n == 0 (done_round 1) at the first, a middle and the last index", ref(1, 500, 150),
          [(0, []), (1, [(at(1, 500) + 30, 30, 40)]), (0, []), (2, [(at(2, 700) + 10, 10, 22)]), (0, [])],
          check=lambda sh, ca, rg: [int(x) for x in sh[:, SH["dp_left"]] + sh[:, SH["dp_right"]] > 0] == [0, 1, 0, 1, 0], n_regs=[0, 1, 0, 1, 0],
          regs={0: whole(at(1, 500), 150)})
    c.add("whole-read seed", "qbeg == 0 and len == l_query: no DP at all; the second chain waits for it and is explained", ref(2, 3000, 150),
          [(2, [(at(2, 3000), 0, 150)]), (2, [(at(2, 3000) + 50, 50, 30)])],
          check=lambda sh, ca, rg: len(ca) == 0 and sh[1, SH["n_dep"]] == 1 and sh[1, SH["skipped"]] == 1, n_regs=[1, 0], regs={0: whole(at(2, 3000), 150)})
    # ---- one chain's seeds
    s = at(1, 4000)
    c.add("qbeg == 0", "no left task", ref(1, 4000, 150), [(1, [(s, 0, 30)])], check=lambda sh, ca, rg: sh[0, SH["dp_left"]] == 0 and sh[0, SH["dp_right"]] == 1,
          n_regs=[1], regs={0: whole(s, 150)})
    c.add("qbeg + len == l_query", "no right task", ref(1, 4000, 150), [(1, [(s + 120, 120, 30)])],
          check=lambda sh, ca, rg: sh[0, SH["dp_left"]] == 1 and sh[0, SH["dp_right"]] == 0, n_regs=[1], regs={0: whole(s, 150)})
    c.add("equal lengths", "all seeds of equal length: visited by index from the top", np.concatenate([ref(1, 100, 50), ref(1, 900, 50), ref(1, 1700, 50)]),
          [(1, [(at(1, 100) + 10, 10, 20), (at(1, 900) + 10, 60, 20), (at(1, 1700) + 10, 110, 20)])],
          check=lambda sh, ca, rg: [int(x) for x in ca[np.r_[True, np.diff(ca[:, CL["seed"]]) != 0], CL["seed"]]] == [2, 1, 0] and sh[0, SH["regs"]] == 3, n_regs=[3])
    c.add("skipped seed", "the second seed lies on the first one's region", ref(1, 4000, 150), [(1, [(s + 20, 20, 40), (s + 100, 100, 25)])],
          check=lambda sh, ca, rg: sh[0, SH["skipped"]] == 1 and sh[0, SH["regs"]] == 1, n_regs=[1], regs={0: whole(s, 150)})
    # an explained seed (q 60, len 19, true diagonal) and a longer seed three bases off the diagonal that was extended before it and overlaps it in the
    # read by 4 = 19 >> 2 bases (kept) or by 3 (skipped).  (The other test of that loop, t.len < s.len * .95, can never hold on this path: seeds are
    # visited by descending score == len, so an extended seed is never shorter than the one in question.)
    for ov, keep in ((4, 1), (3, 0)):
        tq = 60 + 19 - ov
        c.add(f"off-diagonal overlap {ov}", "an explained seed and an extended, overlapping off-diagonal seed: s.len >> 2 == 4 bases of overlap keep it, 3 do not",
              ref(1, 4000, 150), [(1, [(s + 60, 60, 19), (s + tq + 3, tq, 21)])],
              check=lambda sh, ca, rg, keep=keep: sh[0, SH["kept_overlap"]] == keep and sh[0, SH["skipped"]] == 1 - keep and sh[0, SH["regs"]] == 1 + keep, n_regs=[1 + keep])
    for d, n2 in ((15, 0), (16, 1)):
        c.add(f"seedlen0 + {d}", "s.len - seedlen0 at .1 * l_query (explained) and one above it (not looked at)", ref(1, 4000, 150),
              [(1, [(s + 20, 20, 20)]), (1, [(s + 60, 60, 20 + d)])],
              check=lambda sh, ca, rg, n2=n2: sh[1, SH["n_dep"]] == 1 and sh[1, SH["regs"]] == n2 and rg[0, RG["seedlen0"]] == 20, n_regs=[1, n2], regs={0: whole(s, 150)})
    # ---- band: h0 = 100, 10 matches, `gap` reference bases missing from the read, 120 matches
    for gap, tries in ((74, 1), (75, 2), (80, 2)):
        a, x, b, sd = ref(0, 5000, 120), gap, ref(0, 5120 + gap, 10), ref(0, 5130 + gap, 100)
        s = at(0, 5000)
        sc = 100 + 10 - (6 + gap) + 120
        c.add(f"left gap {gap}", "a deletion of 74 (max_off < 75: one try) / 75, 80 (a second band, same score, a.w 200) behind the seed on the left",
              np.concatenate([a, b, sd]), [(0, [(s + 130 + gap, 130, 100)])],
              check=lambda sh, ca, rg, gap=gap, tries=tries: sh[0, SH["band2_left"]] == tries - 1 and len(ca) == tries and ca[0, CL["max_off"]] == gap
              and ca[-1, CL["score"]] == ca[0, CL["score"]] and rg[0, RG["w"]] == 100 * tries,
              n_regs=[1], regs={0: (s, s + 230 + gap, 0, 230, sc, sc, 100 * tries)})
        s = at(0, 6000)
        sd, b, a = ref(0, 6000, 100), ref(0, 6100, 10), ref(0, 6110 + gap, 120)
        c.add(f"right gap {gap}", "the same on the right", np.concatenate([sd, b, a]), [(0, [(s, 0, 100)])],
              check=lambda sh, ca, rg, gap=gap, tries=tries: sh[0, SH["band2_right"]] == tries - 1 and len(ca) == tries and ca[0, CL["max_off"]] == gap
              and ca[-1, CL["score"]] == ca[0, CL["score"]] and rg[0, RG["w"]] == 100 * tries,
              n_regs=[1], regs={0: (s, s + 230 + gap, 0, 230, sc, sc, 100 * tries)})
    c.add("no chains, middle read", "n_chain == 0 between reads that have chains", ref(0, 100, 150), [], check=lambda sh, ca, rg: len(sh) == 0, n_regs=[])
    # ---- ends: one differing base at the last, fifth-last and sixth-last position of each side (seed q 60, len 30)
    s = at(2, 6000)
    for k in (1, 5, 6):   # (at -1 the to-end score is the local one less 4, at -5 equal to it, at -6 it is the maximum itself: the to-end branch every time)
        sc = 150 - 5      # the alignment runs to the end on both sides: one substitution
        c.add(f"left end -{k}", "a differing base at the last / fifth-last / sixth-last position of the left side: gscore against score - 5", _sub(ref(2, 6000, 150), k - 1),
              [(2, [(s + 60, 60, 30)])], check=lambda sh, ca, rg, k=k: sh[0, SH["toend_left"]] == 1 and ca[0, CL["gscore"]] - ca[0, CL["score"]] == (-4 if k == 1 else 0)
              and ca[0, CL["qle"]] == (60 if k == 6 else 60 - k),
              n_regs=[1], regs={0: (s, s + 150, 0, 150, 149 if k == 1 else 145, sc, 100)})
        c.add(f"right end -{k}", "the same on the right", _sub(ref(2, 6000, 150), 150 - k),
              [(2, [(s + 60, 60, 30)])], check=lambda sh, ca, rg, k=k: sh[0, SH["toend_right"]] == 1 and ca[1, CL["gscore"]] - ca[1, CL["score"]] == (-4 if k == 1 else 0)
              and ca[1, CL["qle"]] == (60 if k == 6 else 60 - k),
              n_regs=[1], regs={0: (s, s + 150, 0, 150, 149 if k == 1 else 145, sc, 100)})
    # an inserted base k bases before the right end: gscore = score - 7 + k
    for k, toend in ((2, 0), (3, 1)):
        r = ref(2, 6000, 149)
        ins = (int(ref(2, 6000 + 149 - k, 1)[0]) + 2) & 3
        read = np.concatenate([r[:149 - k], [ins], r[149 - k:]]).astype(np.uint8)
        c.add(f"indel {k} from the end", "an inserted base near the right end puts gscore at score - 5 (clipped) and at score - 4 (to the end)", read,
              [(2, [(s + 60, 60, 30)])], check=lambda sh, ca, rg, k=k, toend=toend: ca[1, CL["gscore"]] == ca[1, CL["score"]] - 7 + k and sh[0, SH["toend_right"]] == toend,
              n_regs=[1], regs={0: (s, s + 149, 0, 150, 149 - k, 149 - 7, 100) if toend else (s, s + 149 - k, 0, 149 - k, 149 - k, 149 - k, 100)})
    # ---- windows: a seed at a contig's first / last base with read left over, on every contig and both strands
    for ctg in (0, 1, 2):
        n = len(g.seqs[ctg])
        junk = rng.integers(0, 4, size=30, dtype=np.uint8)
        for rev in (False, True):
            side = ("left", "right")[rev]   # read from the other strand the contig's first base is the alignment's last
            bit = {(0, False): 1, (0, True): 4, (1, False): 8, (1, True): 8, (2, False): 8, (2, True): 8}[(ctg, rev)]
            c.add(f"contig {ctg} start, strand {int(rev)}", f"a seed at the contig's first base with read in front of it: tlen == 0 on the {side}",
                  np.concatenate([junk, ref(ctg, 0, 120)]), [(ctg, [(at(ctg, 0), 30, 40)])], rev=rev,
                  check=lambda sh, ca, rg, rev=rev, bit=bit: sh[0, SH["tlen0"]] == 1 and ca[0 if not rev else 1, CL["tlen"]] == 0 and sh[0, SH["clamp"]] & bit,
                  n_regs=[1], regs={0: (at(ctg, 0), at(ctg, 0) + 120, 30, 150, 120, 120, 100)})
            side = ("right", "left")[rev]
            bit = {(0, False): 8, (0, True): 8, (1, False): 8, (1, True): 8, (2, False): 2, (2, True): 2}[(ctg, rev)]
            c.add(f"contig {ctg} end, strand {int(rev)}", f"a seed at the contig's last base with read behind it: tlen == 0 on the {side}",
                  np.concatenate([ref(ctg, n - 120, 120), junk]), [(ctg, [(at(ctg, n - 40), 80, 40)])], rev=rev,
                  check=lambda sh, ca, rg, rev=rev, bit=bit: sh[0, SH["tlen0"]] == 1 and ca[1 if not rev else 0, CL["tlen"]] == 0 and sh[0, SH["clamp"]] & bit,
                  n_regs=[1], regs={0: (at(ctg, n - 120), at(ctg, n), 0, 120, 120, 120, 100)})
    c.add("short window", "a window cut to 0 < tlen < qlen", np.concatenate([rng.integers(0, 4, size=20, dtype=np.uint8), ref(1, 0, 130)]),
          [(1, [(at(1, 10), 30, 40)])], check=lambda sh, ca, rg: sh[0, SH["tlen_short"]] == 1 and ca[0, CL["tlen"]] == 10 and ca[0, CL["qlen"]] == 30, n_regs=[1])
    # ---- task lengths at every class boundary, and the longest a read allows; two differing bases keep every task a DP
    for ql in (31, 32, 47, 48, 63, 64, 95, 96, 127, 128, 159, 160, 229):
        s = at(0, 8000)
        c.add(f"left qlen {ql}", "a left task at a length-class boundary", _sub(ref(0, 8000, 250), 3, 9), [(0, [(s + ql, ql, 20)])],
              check=lambda sh, ca, rg, ql=ql: ca[0, CL["qlen"]] == ql and ca[0, CL["side"]] == 0, n_regs=[1])
        c.add(f"right qlen {ql}", "a right task at a length-class boundary", _sub(ref(0, 8000, 250), 240, 246), [(0, [(s + 230 - ql, 230 - ql, 20)])],
              check=lambda sh, ca, rg, ql=ql: ca[-1, CL["qlen"]] == ql and ca[-1, CL["side"]] == 1, n_regs=[1])
    s = at(0, 8000)
    c.add("left qlen 249", "the longest left task a read allows", _sub(ref(0, 8000, 250), 3, 9), [(0, [(s + 249, 249, 1)])],
          check=lambda sh, ca, rg: len(ca) == 1 and ca[0, CL["qlen"]] == 249 and ca[0, CL["side"]] == 0, n_regs=[1])
    c.add("right qlen 249", "the longest right task a read allows", _sub(ref(0, 8000, 250), 240, 246), [(0, [(s, 0, 1)])],
          check=lambda sh, ca, rg: len(ca) == 1 and ca[0, CL["qlen"]] == 249 and ca[0, CL["side"]] == 1, n_regs=[1])
    c.add("no chains, last read", "n_chain == 0 at the last read", ref(0, 100, 150), [], check=lambda sh, ca, rg: len(sh) == 0, n_regs=[])
    return c


def build_nodp(g):
    """One read, no DP anywhere: the round loop's `nt == 0` continue."""
    c = Cases(g, "no DP")
    s = c.at(2, 3000)
    c.add("whole-read seed alone", "round 2 leaves a waiting chain and queues no task", c.ref(2, 3000, 150), [(2, [(s, 0, 150)]), (2, [(s + 50, 50, 30)])],
          check=lambda sh, ca, rg: len(ca) == 0 and sh[1, SH["n_dep"]] == 1, n_regs=[1, 0], regs={0: (s, s + 150, 0, 150, 150, 150, 100)})
    return c


def build_lanes(g, n_active):
    """n_active chains that all queue a task in round 2 (63, 64, 65: a wavefront's ballots not full, full, and one lane into the next)."""
    c = Cases(g, f"active={n_active}")
    for k in range(n_active):
        ql = (31, 32, 47, 64, 95, 128, 160)[k % 7]
        s = c.at(k % 3, 300 + 7 * k)
        c.add(f"lane {k}", "one chain, a left task that two differing bases keep a DP", _sub(c.ref(k % 3, 300 + 7 * k, 200), 2, 5), [(k % 3, [(s + ql, ql, 25)])],
              check=lambda sh, ca, rg, ql=ql: ca[0, CL["qlen"]] == ql, n_regs=[1])
    return c


def build_big(g, main, n_chains=4100):
    """The main batch's reads over and over until the batch holds n_chains chains: one workgroup strides (grid_cap = 1: 64 lanes, 65 steps)."""
    c = Cases(g, "big")
    k = 0
    while sum(len(r["chains"]) for r in c.reads) < n_chains:
        r = main.reads[k % len(main.reads)]
        c.reads.append(dict(r, name=f"{r['name']} #{k // len(main.reads)}"))
        k += 1
    return c


def first_wavefront(batch, ora):
    """What the first 64 chains of a batch do in round 2 (one wavefront of KExtStep's ballots), from the restatement's rows: the length classes of the
    tasks they queue, how many wait, how many finish without a task, how many are empty"""
    classes, wait, finish, empty, g = set(), 0, 0, 0, 0
    for r, a in zip(batch.reads, ora["reads"]):
        for ci in range(len(a["sh"])):
            if g < 64:
                ca = _calls_of(a["calls"], ci)
                if r["ch"][ci, 2] == 0:
                    empty += 1
                elif a["sh"][ci, SH["n_dep"]]:
                    wait += 1
                elif len(ca) == 0:
                    finish += 1
                else:
                    classes.add(ext_class(int(ca[0, CL["qlen"]])))
            g += 1
    return dict(classes=sorted(classes), wait=wait, finish=finish, empty=empty)


def build_all():
    g = Genome()
    main = build_main(g)
    return dict(genome=g, batches=[main, build_nodp(g)] + [build_lanes(g, n) for n in (63, 64, 65)], big=build_big(g, main))


# ------------------------------------------------------------------------------------------------------------------------------------------
def oracle(o, batch):
    """The restatement's answer for a batch: per read ora_chain2aln (regions, calls, shapes) and mem_sort_dedup_patch on the regions."""
    rows = batch.rows()
    out = []
    for r in batch.reads:
        res = o.chain2aln(r["read"], r["ch"], r["sd"], FRAC_REP_BITS)
        assert res is not None, (batch.name, r["name"], "refused")
        regs, calls, sh = res
        out.append(dict(regs=regs, calls=calls, sh=sh, core=o.sort_dedup_patch(r["read"], regs)))
    return dict(rows=rows, reads=out)


def check_edges(batch, ora):
    """Every case shows its edge in the restatement's rows, and gives what was written down for it.  -> the number of cases held"""
    for r, a in zip(batch.reads, ora["reads"]):
        regs, calls, sh = a["regs"], a["calls"], a["sh"]
        what = (batch.name, r["name"], r["edge"])
        assert r["check"] is None or bool(r["check"](sh, calls, regs)), (what, sh.tolist(), calls.tolist(), regs[:, :12].tolist())
        assert int(sh[:, SH["regs"]].sum()) == len(regs), what
        if r["n_regs"] is not None:
            assert [int(x) for x in sh[:, SH["regs"]]] == list(r["n_regs"]), (what, sh[:, SH["regs"]].tolist())
        for k, v in (r["regs"] or {}).items():
            got = tuple(int(regs[k, RG[f]]) for f in ("rb", "re", "qb", "qe", "score", "truesc", "w")[:len(v)])
            assert got == tuple(int(x) for x in v), (what, k, got, v)
        assert (regs[:, RG["frac_rep_bits"]] == FRAC_REP_BITS).all() and (regs[:, RG["secondary"]] == 0).all(), what
    return len(batch.reads)


def base_at(g, L, p):
    """ref_base of arx_dev.h on the doubled coordinate"""
    fwd = getattr(g, "_fwd", None)
    if fwd is None:
        fwd = g._fwd = np.concatenate(g.seqs)
    return int(fwd[p]) if p < L else 3 - int(fwd[2 * L - 1 - p])


def closed_calls(batch, ora):
    """Which calls of the restatement's lists the stage answers itself (dev_sw.h ext_closed_form_pairwise: tlen >= qlen > 0, h0 >= 5, no ambiguous
    base, at most one differing pair along the diagonal) -> their number"""
    n = 0
    for r, a in zip(batch.reads, ora["reads"]):
        for ca in a["calls"]:
            rb, qb, ln, _ = (int(x) for x in r["sd"][int(r["ch"][int(ca[CL["chain"]]), 3]) + int(ca[CL["seed"]])])
            ql, tl, left = int(ca[CL["qlen"]]), int(ca[CL["tlen"]]), ca[CL["side"]] == 0
            if ql <= 0 or tl < ql or ca[CL["h0"]] < 5:
                continue
            q = [int(r["read"][qb - 1 - j]) if left else int(r["read"][qb + ln + j]) for j in range(ql)]
            t = [base_at(batch.g, batch.L, rb - 1 - j if left else rb + ln + j) for j in range(ql)]
            if max(q) <= 3 and sum(1 for x, y in zip(q, t) if x != y) <= 1:
                n += 1
    return n


def check_device(batch, ora, dev, closed):
    """dev: api.selftest_ext_stage's dict.  Everything without a tolerance: the gathered regions are ora_chain2aln's rows bit for bit (frac_rep's bits
    and w included), the core regions mem_sort_dedup_patch's on those rows; the task count is the call list's length (less the calls the stage answers
    itself with the closed form on); with it off the census's class totals are the list binned by ext_class(qlen); n_act never rises and ends at 0;
    every chain's n_regs is the shape row's; a chain waits for every earlier chain whose window holds one of its seeds."""
    rd = ora["reads"]
    assert dev["err"] == 0
    exp_ext = np.concatenate([a["regs"] for a in rd]).reshape(-1, 20)
    exp_core = np.concatenate([a["core"] for a in rd]).reshape(-1, 20)
    assert dev["ext_off"].tolist() == np.concatenate([[0], np.cumsum([len(a["regs"]) for a in rd])]).tolist()
    bad = np.flatnonzero((dev["ext_regs"] != exp_ext).any(axis=1))
    assert len(bad) == 0, (batch.name, "gathered regions", int(bad[0]), dev["ext_regs"][bad[0]].tolist(), exp_ext[bad[0]].tolist())
    assert dev["core_off"].tolist() == np.concatenate([[0], np.cumsum([len(a["core"]) for a in rd])]).tolist()
    bad = np.flatnonzero((dev["core_regs"] != exp_core).any(axis=1))
    assert len(bad) == 0, (batch.name, "core regions", int(bad[0]), dev["core_regs"][bad[0]].tolist(), exp_core[bad[0]].tolist())
    calls = np.concatenate([a["calls"] for a in rd]).reshape(-1, len(CL))
    sh = np.concatenate([a["sh"] for a in rd]).reshape(-1, len(SH))
    rounds = dev["rounds"]
    if closed:
        assert dev["n_ext_tasks"] == len(calls) - closed_calls(batch, ora), (dev["n_ext_tasks"], len(calls))
    else:
        assert dev["n_ext_tasks"] == len(calls), (dev["n_ext_tasks"], len(calls))
        assert rounds[:, 2:].sum(axis=0).tolist() == np.bincount([ext_class(int(x)) for x in calls[:, CL["qlen"]]], minlength=7).tolist()
    assert int(rounds[:, 2:].sum()) == dev["n_ext_tasks"] and dev["ext_rounds"] == int((rounds[:, 2:].sum(axis=1) > 0).sum())
    n_live = int((ora["rows"]["chains"][:, 2] > 0).sum())
    n_act = np.concatenate([[n_live], rounds[:, 1]]) if len(rounds) else np.array([n_live])
    assert (np.diff(n_act) <= 0).all() and n_act[-1] == 0, n_act.tolist()
    assert rounds[:, 0].tolist() == list(range(2, 2 + len(rounds)))
    assert dev["n_regs"].tolist() == sh[:, SH["regs"]].tolist()
    done, chains = dev["done_round"], ora["rows"]["chains"]
    assert ((done == 1) == (chains[:, 2] == 0)).all() and (done >= 1).all()
    g0 = 0
    for r, a in zip(batch.reads, rd):       # the dependency rule, from the windows and the seed rows themselves
        for ci in range(len(a["sh"])):
            sd = r["sd"][int(r["ch"][ci, 3]):int(r["ch"][ci, 3] + r["ch"][ci, 2])]
            deps = [k for k in range(ci) if r["ch"][k, 2] > 0 and ((sd[:, 0] >= a["sh"][k, SH["rmax0"]]) & (sd[:, 0] + sd[:, 2] <= a["sh"][k, SH["rmax1"]])).any()]
            assert len(deps) == a["sh"][ci, SH["n_dep"]] and (not deps or deps[-1] == a["sh"][ci, SH["dep_last"]])
            for k in deps:
                assert done[g0 + ci] > done[g0 + k] >= 2, (batch.name, r["name"], ci, k, done[g0:g0 + len(a["sh"])].tolist())
        g0 += len(a["sh"])
    return dict(calls=len(calls), chains=len(chains), regions=len(exp_ext), core=len(exp_core), rounds=len(rounds))


def run_device(ref, batch, ora, **kw):
    from arachne_amd import api
    w = ora["rows"]
    return api.selftest_ext_stage(ref, w["seqs"], w["lens"], w["n_chain"], w["chains"], w["n_seed"], w["seeds"], w["frb"], **kw)

"""Hand-planted inputs of the CIGAR stage (arx_selftest_reg2aln, the restatement's ora_reg2aln, the reference's mem_reg2aln): a 60 kb genome of
three contigs without ambiguous bases, reads of 30..255 bases with planted substitutions, insertions and deletions, and region rows written
directly -- rb / re / qb / qe from where the edits were planted, truesc and w chosen freely to steer the band.  mem_reg2aln is a pure function
of (region row, read, index), so every such row is legal input.

How the band is steered (bwamem.c:792-799, 1098-1113; bwa.c:150-160), with m = min(l1, l2), d = |l2 - l1|:
  w0 = max(m - truesc - 4, d), unless l1 == l2 and l1 - truesc < 12 (then 0: the gap-free rule); w0 > 100 becomes min(w0, row w); each call
  caps it at 400 and doubles it; bwa_gen_cigar2 runs ksw_global2 with w = max(min((max_gap + d + 1) >> 1, w_), d + 3), max_gap =
  max(1, ((l1 + 1) >> 1) - 5), over n_col = min(l1, 2 w + 1) columns.  band=a below sets truesc = m - 4 - a.

Everything a test asserts about the SHAPE of a case comes from the restatement's shape rows (expected()), never from this file's intentions."""
import os
import tempfile

import numpy as np

from arachne_amd import api, synth

CONTIG_LENS = (30011, 20003, 10007)
REG_W = 20
OPT_W, NW_T_CAP, MAX_LEN = 100, 1024, 255
COL = {n: i for i, n in enumerate(["rb", "re", "qb", "qe", "rid", "score", "truesc", "sub", "alt_sc", "csub", "sub_n", "w", "seedcov", "secondary", "secondary_all",
                                   "seedlen0", "n_comp", "is_alt", "frac_rep_bits", "pad"])}


def _rc(a):
    a = np.asarray(a, dtype=np.uint8)
    return np.where(a < 4, 3 - a, 4).astype(np.uint8)[::-1]


class Builder:
    """Reads with their region slots.  add_read() appends one read; every entry of `rows` is one used region."""

    def __init__(self, seed=20240611):
        self.rng = np.random.default_rng(seed)
        self.seqs = [self.rng.integers(0, 4, size=n, dtype=np.uint8) for n in CONTIG_LENS]
        self.off = np.concatenate([[0], np.cumsum(CONTIG_LENS)]).astype(np.int64)
        self.L = int(self.off[-1])
        self.reads, self.cap, self.rows, self.tags = [], [], [], []   # rows / tags: per read a list

    def genome(self):
        return synth.Genome([f"ctg{i + 1}" for i in range(len(self.seqs))], self.seqs, [False] * len(self.seqs))

    def plant(self, ctg, s, script, clip5=0, clip3=0):
        """Walk contig ctg from s along script -> (read, qb, qe, s, e): ('M', n) copies, ('X', n) n substituted bases, ('I', n) n inserted bases,
        ('D', n) skips n reference bases, ('J', n) n random bases over n reference bases, ('N', n) n ambiguous bases over n reference bases."""
        ref, rng, p, q = self.seqs[ctg], self.rng, s, []
        for op, n in script:
            if op == "M":
                q.append(ref[p:p + n]); p += n
            elif op == "X":
                q.append((ref[p:p + n] + rng.integers(1, 4, size=n, dtype=np.uint8)) & 3); p += n
            elif op == "I":
                q.append(rng.integers(0, 4, size=n, dtype=np.uint8))
            elif op == "D":
                p += n
            elif op == "J":
                q.append(rng.integers(0, 4, size=n, dtype=np.uint8)); p += n
            elif op == "N":
                q.append(np.full(n, 4, dtype=np.uint8)); p += n
            else:
                raise ValueError(op)
        assert p <= len(ref), (ctg, s, p)
        core = np.concatenate(q).astype(np.uint8)
        read = np.concatenate([rng.integers(0, 4, size=clip5, dtype=np.uint8), core, rng.integers(0, 4, size=clip3, dtype=np.uint8)]).astype(np.uint8)
        assert 1 <= len(read) <= MAX_LEN, len(read)
        return read, clip5, clip5 + len(core), s, p

    def row(self, ctg, s, e, qb, qe, l_read, rev, band=None, truesc=None, w=0, **kw):
        l1, l2 = qe - qb, e - s
        if truesc is None:
            truesc = min(l1, l2) - 4 - (0 if band is None else band)
        r = np.zeros(REG_W, dtype=np.int64)
        rb, re = int(self.off[ctg]) + s, int(self.off[ctg]) + e
        if rev:
            rb, re, qb, qe = 2 * self.L - re, 2 * self.L - rb, l_read - qe, l_read - qb
        r[COL["rb"]], r[COL["re"]], r[COL["qb"]], r[COL["qe"]] = rb, re, qb, qe
        r[COL["rid"]], r[COL["truesc"]], r[COL["w"]] = ctg, truesc, w
        r[COL["score"]], r[COL["secondary"]], r[COL["n_comp"]], r[COL["seedcov"]], r[COL["seedlen0"]] = max(truesc, 1), -1, 1, min(l1, l2) >> 1, 19
        for k, v in kw.items():
            r[COL[k]] = v
        return r

    def add_read(self, read, rows, tags, spare=0):
        assert len(rows) == len(tags)
        self.reads.append(np.asarray(read, dtype=np.uint8)); self.cap.append(len(rows) + spare); self.rows.append(list(rows)); self.tags.append(list(tags))

    def empty_read(self, n=40):
        """A read with no region slot at all (capacity 0)."""
        self.add_read(self.rng.integers(0, 4, size=n, dtype=np.uint8), [], [])

    def case(self, tag, ctg, s, script, clip5=0, clip3=0, rev=False, steer=({},), spare=0, tail_d=0):
        """One read planted at (ctg, s) and one region per entry of steer (keyword arguments of row()).  tail_d = k: the script ends in a deletion of k
        bases behind a match run; s moves on until the last matched base differs from the region's last base (otherwise "... k D 1 M" scores the
        same and the traceback, which prefers M, takes it: no trailing deletion)."""
        if tail_d:
            n = sum(k for op, k in script if op != "I")
            while self.seqs[ctg][s + n - 1 - tail_d] == self.seqs[ctg][s + n - 1]:
                s += 1
        read, qb, qe, s, e = self.plant(ctg, s, script, clip5, clip3)
        rows = [self.row(ctg, s, e, qb, qe, len(read), rev, **st) for st in steer]
        self.add_read(_rc(read) if rev else read, rows, [tag] * len(rows), spare)

    def both(self, tag, ctg, s, script, **kw):
        for rev in (False, True):
            self.case(tag + ("-" if rev else "+"), ctg, s + (997 if rev else 0), script, rev=rev, **kw)


def pair_edits(k1, k2=None, gap=40):
    """An insertion of k1 bases and, gap bases on, a deletion of k1 (then the same with k2): the diagonal leaves by k and comes back, so only a band
    of at least k finds it."""
    sc = [("M", 30), ("I", k1), ("M", gap), ("D", k1), ("M", 30)]
    if k2:
        sc += [("I", k2), ("M", gap), ("D", k2), ("M", 30)]
    return sc


def indel_ladder(n_indels, run=15, lead=None):
    sc = [] if lead is None else [lead]
    for i in range(n_indels):
        sc += [("M", run), ("I" if i % 2 == 0 else "D", 1)]
    return sc + [("M", run)]


def build_main():
    """The main batch -> Builder"""
    b = Builder()
    b.empty_read()
    b.empty_read(30)
    # ---- the gap-free rule (pipeline.h KReg2Aln mode 0)
    for rev in (False, True):
        sfx = "-" if rev else "+"
        b.case("gapfree loss 11" + sfx, 0, 100 + 500 * rev, [("M", 60), ("X", 1), ("M", 59)], rev=rev, steer=[dict(truesc=120 - 11)])
        b.case("queued loss 12" + sfx, 0, 1200 + 500 * rev, [("M", 60), ("X", 1), ("M", 59)], rev=rev, steer=[dict(truesc=120 - 12)])
        b.case("unequal loss 0" + sfx, 0, 2200 + 500 * rev, [("M", 60), ("D", 2), ("M", 60)], rev=rev, steer=[dict(truesc=120)])
        b.case("gapfree second call" + sfx, 0, 3200 + 500 * rev, [("M", 40), ("X", 1), ("M", 40), ("X", 1), ("M", 38)], rev=rev, steer=[dict(truesc=120 - 5)])
        b.case("queued shortcut" + sfx, 0, 4200 + 500 * rev, [("M", 60), ("X", 3), ("M", 57)], rev=rev, steer=[dict(truesc=120 - 4 - 150, w=0)])
    b.empty_read()
    # ---- first-band classes: n_col = l1 (a deletion wide enough that 2 (d + 3) + 1 >= l1) and n_col = 2 w + 1
    for l1, d in ((16, 5), (17, 6), (32, 13), (33, 14), (64, 29), (65, 30), (128, 61), (129, 62), (200, 97), (230, 115)):
        h = l1 // 2
        pad = max(0, 30 - l1 + 1) // 2
        b.both(f"n_col=l1={l1}", 1, 300 + 40 * l1, [("M", h), ("D", d), ("M", l1 - h)], clip5=pad, clip3=pad, steer=[dict(band=d)])
    for a, d in ((7, 1), (8, 0), (15, 0), (16, 0), (31, 0), (32, 0), (63, 4), (64, 4)):   # (l1 == l2 and a < 8 would be the gap-free rule)
        sc = [("M", 100), ("X", 1), ("M", 60)] + ([("D", d)] if d else [("X", 1)]) + [("M", 94 if d else 93)]
        b.both(f"n_col=2w+1 w={a}", 1, 2000 + 200 * a, sc, steer=[dict(band=a)])
    # ---- retries: one, two and three calls; the stop on an equal score; the cap of 400 at each call; the clamp by the row's w
    for rev in (False, True):
        sfx = "-" if rev else "+"
        b.case("pairs 10/20" + sfx, 2, 200 + 1500 * rev, pair_edits(10, 20), rev=rev, spare=2,
               # (l1 == l2 here, so bands 3 and 5 fall under the gap-free rule: one M run over both pairs, finished inline, called twice)
               steer=[dict(band=8), dict(band=12), dict(band=3), dict(band=30), dict(band=8, sub=5, csub=9), dict(band=5, secondary=0, sub=9, csub=5)])
        b.case("pair 40 never found" + sfx, 2, 3200 + 1500 * rev, pair_edits(40, gap=30), rev=rev, steer=[dict(band=4), dict(band=9)])
        junk = [("M", 20), ("J", 215), ("M", 20)]
        b.case("junk 255, cap at call 1/2/3" + sfx, 2, 5200 + 1500 * rev, junk, rev=rev, spare=1,
               steer=[dict(truesc=255 - 4 - 450, w=500), dict(truesc=255 - 4 - 450, w=400), dict(truesc=255 - 4 - 200, w=300), dict(truesc=255 - 4 - 300, w=200),
                      dict(truesc=255 - 4 - 150, w=120, is_alt=1, alt_sc=77), dict(truesc=255 - 4 - 150, w=180), dict(truesc=255 - 4 - 100, w=7)])
        # d = 100: the band is 103 at w_ = 100 and 112 from w_ = 200 on; the 8-base pair around the deletion needs 108
        b.case("cap at call 3" + sfx, 0, 8000 + 1500 * rev, [("M", 50), ("D", 8), ("M", 42), ("D", 100), ("M", 50), ("I", 8), ("M", 105)], rev=rev,
               steer=[dict(truesc=255 - 104, w=0)])
    b.empty_read()
    # ---- junk between two anchors: the score stays far below truesc, so every band is tried (w_ = a, 2a, 4a).  The second call always fits the class
    # kernel (its HI is the doubled tiling); the third leaves it in classes 0..2 -- a punt -- and cannot in class 3 (16 x 16 columns hold any read)
    for name, L1, d, bands in (("class 0", 120, 1, (4, 5, 6, 7)), ("class 1", 200, 0, (8, 10, 12, 15)), ("class 2", 255, 10, (17, 20, 25, 31)), ("class 3", 255, 10, (33, 40, 62))):
        for rev in (False, True):
            sc = [("M", 15), ("J", L1 - 30)] + ([("D", d)] if d else []) + [("M", 15)]
            read, qb, qe, s, e = b.plant(1, 500 + 2300 * rev + 300 * int(name[-1]), sc)
            rows = [b.row(1, s, e, qb, qe, len(read), rev, band=a) for a in bands]
            b.add_read(_rc(read) if rev else read, rows, [f"{name} junk" + ("-" if rev else "+")] * len(rows), spare=1)
    # ---- squeeze, clips, geometry
    for rev in (False, True):
        sfx = "-" if rev else "+"
        o = 700 * rev
        b.case("lead D1" + sfx, 0, 12000 + o, [("D", 1), ("M", 100)], clip5=5, rev=rev, steer=[dict(band=6)])
        b.case("lead D12" + sfx, 0, 12200 + o, [("D", 12), ("M", 100)], clip3=7, rev=rev, steer=[dict(band=14)])
        b.case("trail D" + sfx, 0, 12400 + o, [("M", 100), ("D", 5)], rev=rev, steer=[dict(band=8)], tail_d=5)
        b.case("lead and trail D" + sfx, 0, 12600 + o, [("D", 6), ("M", 100), ("D", 4)], clip5=3, clip3=4, rev=rev, steer=[dict(band=12)], tail_d=4)
        b.case("interior D" + sfx, 0, 12800 + o, [("M", 50), ("D", 7), ("M", 50)], rev=rev, steer=[dict(band=9)])
        b.case("lead I" + sfx, 0, 13000 + o, [("I", 6), ("M", 100)], rev=rev, steer=[dict(band=8)])
        b.case("clips none" + sfx, 0, 14600 + o, [("M", 50), ("D", 2), ("M", 50)], rev=rev, steer=[dict(band=4)])
        b.case("clip 5'" + sfx, 0, 14800 + o, [("M", 50), ("D", 2), ("M", 50)], clip5=11, rev=rev, steer=[dict(band=4)])
        b.case("clip 3'" + sfx, 0, 15000 + o, [("M", 50), ("D", 2), ("M", 50)], clip3=13, rev=rev, steer=[dict(band=4)])
        b.case("clips both" + sfx, 0, 15200 + o, [("M", 50), ("I", 2), ("M", 50)], clip5=17, clip3=19, rev=rev, steer=[dict(band=4)])
        b.case("ambiguous in M" + sfx, 0, 15400 + o, [("M", 40), ("N", 2), ("M", 30), ("D", 1), ("M", 30)], rev=rev, steer=[dict(band=6)])
        b.case("read of 30" + sfx, 0, 15600 + o, [("M", 14), ("I", 1), ("M", 15)], rev=rev, steer=[dict(band=5)])
        # contig edges: the first base of the first contig and the last base of the last one (forward: rb == 0, re == l_pac; reverse: re == 2 l_pac, rb == l_pac)
        b.case("first contig start" + sfx, 0, 0, [("M", 60), ("I", 2), ("M", 60)], clip3=5, rev=rev, steer=[dict(band=5)])
        b.case("first contig end" + sfx, 0, CONTIG_LENS[0] - 122, [("M", 60), ("D", 2), ("M", 60)], rev=rev, steer=[dict(band=5)])
        b.case("last contig start" + sfx, 2, 0, [("M", 60), ("D", 3), ("M", 60)], rev=rev, steer=[dict(band=5)])
        b.case("last contig end" + sfx, 2, CONTIG_LENS[2] - 121, [("M", 60), ("I", 1), ("M", 61)], clip5=5, rev=rev, steer=[dict(band=5)])
        b.case("lead D at contig start" + sfx, 1 if not rev else 2, 0, [("D", 9), ("M", 90)], clip5=4, rev=rev, steer=[dict(band=11)])
        b.case("trail D at contig end" + sfx, 1, CONTIG_LENS[1] - 96, [("M", 90), ("D", 6)], rev=rev, steer=[dict(band=9)], tail_d=6)
        b.case("core 14 with both clips" + sfx, 1, 6000 + o, indel_ladder(6, lead=("I", 2)), clip5=3, clip3=3, rev=rev, steer=[dict(band=6)])
        b.case("core 14 with lead D" + sfx, 1, 6400 + o, indel_ladder(6, lead=("D", 3)), clip5=3, clip3=3, rev=rev, steer=[dict(band=8)])
        b.case("core 13" + sfx, 1, 6800 + o, indel_ladder(6), rev=rev, steer=[dict(band=8)])
    b.empty_read()
    # ---- long regions: the longest the 16-lane kernel stages, and one base more (the one-thread path)
    for rev in (False, True):
        for l2 in (NW_T_CAP, NW_T_CAP + 1):
            b.case(f"re-rb={l2}" + ("-" if rev else "+"), 0, 17000 + 3000 * rev + 1500 * (l2 - NW_T_CAP), [("M", 50), ("D", l2 - 100), ("M", 50)], rev=rev, steer=[dict(band=l2 - 100)])
    # ---- slices: 66 regions of 255 x 255 next to each other in the queue, every one run once at the widest band its slice is sized for
    for i in range(66):
        rev = i % 2 == 1
        b.case("slice 255x255" + ("-" if rev else "+"), i % 3, 300 + 280 * (i // 3),
               [("M", 60), ("I", 20), ("M", 50), ("D", 20), ("M", 30), ("X", 2), ("M", 93)], rev=rev, steer=[dict(truesc=255 - 4 - 300, w=62 + (i % 5))])
    # ---- slot overflows: 15 core operations (one pass more), 30 (fits 32) and 31 (a third pass, 64 words)
    for rev in (False, True):
        sfx = "-" if rev else "+"
        o = 900 * rev
        b.case("core 15" + sfx, 1, 8000 + o, indel_ladder(7), rev=rev, steer=[dict(band=6)])
        b.case("core 30" + sfx, 1, 9800 + o, indel_ladder(14, run=14, lead=("I", 2)), clip5=2, clip3=2, rev=rev, steer=[dict(band=6)])
        b.case("core 31" + sfx, 2, 7800 + o, indel_ladder(15, run=14), rev=rev, steer=[dict(band=6)])
    b.empty_read()
    return b


def build_small():
    """The batch of the call of its own: band class lists of 1, 3, 4 and 5 regions (a partial, a full and a spilling wavefront of four groups), and
    one long region whose matrix the one-thread path cannot hold (ERR_POOL_OVERFLOW; the tag says which)."""
    b = Builder(seed=77)
    b.empty_read()
    sc = [("M", 100), ("X", 1), ("M", 60), ("D", 4), ("M", 94)]
    for a, n in ((5, 1), (12, 3), (20, 4), (40, 5)):
        for i in range(n):
            b.case(f"class list of {n}", 0, 1000 + 300 * (a + i), sc, rev=i % 2 == 1, steer=[dict(band=a)])
    b.case("beyond z_cap", 1, 2000, [("M", 75), ("D", 1025 - 150), ("M", 75)], steer=[dict(band=900)])
    b.case("long, inside z_cap", 1, 5000, [("M", 50), ("D", 1030 - 100), ("M", 50)], rev=True, steer=[dict(band=940)])
    b.case("gap-free", 2, 100, [("M", 200)], steer=[dict(truesc=200)])
    return b


def flatten(b, reads=None):
    """-> dict(seqs, lens, cap, n_regs, regs (one row per slot), rows (one per used region), tags, read_of) for the stage's entry and the restatement."""
    idx = list(range(len(b.reads))) if reads is None else list(reads)
    lens = np.array([len(b.reads[i]) for i in idx], dtype=np.int32)
    cap = np.array([b.cap[i] for i in idx], dtype=np.int32)
    n_regs = np.array([len(b.rows[i]) for i in idx], dtype=np.int32)
    slots, used, tags, read_of = [], [], [], []
    for k, i in enumerate(idx):
        for j in range(b.cap[i]):
            if j < len(b.rows[i]):
                slots.append(b.rows[i][j]); used.append(b.rows[i][j]); tags.append(b.tags[i][j]); read_of.append(k)
            else:
                slots.append(np.zeros(REG_W, dtype=np.int64))
    return dict(seqs=np.concatenate([b.reads[i] for i in idx]), lens=lens, cap=cap, n_regs=n_regs, regs=np.array(slots, dtype=np.int64).reshape(-1, REG_W),
                rows=np.array(used, dtype=np.int64).reshape(-1, REG_W), tags=tags, read_of=np.array(read_of, dtype=np.int64), reads=[b.reads[i] for i in idx], ids=idx)


def write_index(b, lib_path=None):
    d = tempfile.mkdtemp(prefix="arx_cigar_cases_")
    fa = os.path.join(d, "g.fa")
    b.genome().write_fasta(fa)
    if lib_path is None:
        api.index_build(fa, fa)
    else:
        api.index_build(fa, fa, lib_path=lib_path)
    return fa


def expected(drv, flat, with_shape=True):
    """The restatement (or, with_shape=False, the compiled reference) on every used region -> dict(alns (n x 12, cigar_off filled in), cigars, shapes)."""
    alns, cigs, shapes, off = [], [], [], 0
    for row, r in zip(flat["rows"], flat["read_of"]):
        out = drv.reg2aln(flat["reads"][int(r)], row)
        a, cg = out[0].copy(), out[1]
        a[8] = off
        off += len(cg)
        alns.append(a); cigs.append(cg)
        if with_shape:
            shapes.append(out[2])
    return dict(alns=np.array(alns, dtype=np.int64).reshape(-1, 12), cigars=np.concatenate(cigs).astype(np.uint32) if cigs else np.zeros(0, np.uint32),
                shapes=np.array(shapes, dtype=np.int64) if with_shape else None)


# ---- what the restatement's shape rows say the product must do (hip_nw_coop.h, pipeline.h), restated here without the product's code
def tiling(n_col):
    return 1 if n_col <= 16 else 2 if n_col <= 32 else 4 if n_col <= 64 else 8 if n_col <= 128 else 16


def band_class(n_col):
    return {1: 0, 2: 1, 4: 2, 8: 3, 16: 4}[tiling(n_col)]


def census_from_shapes(flat, shapes):
    """From the rows and the restatement alone: inline gap-free regions, long ones, queued ones per class of the first band's n_col, punts (an
    executed try needs more than 16 x HI columns of the class kernel), and per queued region the bytes of matrix its widest try writes."""
    rows = flat["rows"]
    l1, l2 = rows[:, COL["qe"]] - rows[:, COL["qb"]], rows[:, COL["re"]] - rows[:, COL["rb"]]
    inline = (l1 == l2) & (l1 - rows[:, COL["truesc"]] < 12)
    big = ~inline & (l2 > NW_T_CAP)
    queued = ~inline & ~big
    n_cols = shapes[:, 7:10]
    klass = np.array([band_class(int(c)) for c in n_cols[:, 0]])
    hi = np.array([2, 4, 8, 16, 16])[klass] * 16
    punt = queued & (n_cols.max(axis=1) > hi)
    need = np.zeros(len(rows), dtype=np.int64)
    for g in np.flatnonzero(queued):
        lo = 1 << klass[g]
        need[g] = max(16 * max(lo, tiling(int(c))) for c in n_cols[g, :int(shapes[g, 0])]) * int(l2[g])
    return dict(inline=inline, big=big, queued=queued, klass=klass, punt=punt, need_bytes=need, per_class=[int((queued & (klass == c)).sum()) for c in range(5)])


ALN_COLS = [("pos", 0), ("rid", 1), ("flag", 2), ("is_rev", 3), ("is_alt", 4), ("NM", 6), ("n_cigar", 7), ("cigar_off", 8), ("score", 9), ("sub", 10), ("alt_sc", 11)]
ERR_POOL_OVERFLOW, ERR_CIGAR_OVERFLOW = 4, 8


def check_stage(dev, flat, exp, skip=()):
    """dev: api.selftest_reg2aln's dict; exp: expected().  reg_off, every Aln field (parity.ALN_MAP's and the CIGAR offset) and every CIGAR word, bit
    for bit.  skip: regions whose record the stage must have refused (rid -1, no CIGAR; their words are taken out of the expected CIGARs)."""
    want_off = np.concatenate([[0], np.cumsum(flat["n_regs"])])
    assert (dev["reg_off"].astype(np.int64) == want_off).all(), "compacted reg_off differs"
    a, cg = exp["alns"].copy(), exp["cigars"]
    if len(skip):
        keep = np.ones(len(cg), dtype=bool)
        for g in skip:
            keep[a[g, 8]:a[g, 8] + a[g, 7]] = False
            assert dev["alns"]["rid"][g] == -1 and dev["alns"]["n_cigar"][g] == 0, f"region {g} ({flat['tags'][g]}) should have been refused"
        cg = cg[keep]
        n = a[:, 7].copy()
        n[list(skip)] = 0
        a[:, 8] = np.concatenate([[0], np.cumsum(n)[:-1]])
    ok = np.ones(len(a), dtype=bool)
    ok[list(skip)] = False
    for name, col in ALN_COLS:
        d = dev["alns"][name].astype(np.int64)
        bad = np.flatnonzero((d != a[:, col]) & ok)
        assert len(bad) == 0, f"aln field {name} differs at region {bad[0]} ({flat['tags'][bad[0]]}): stage {d[bad[0]]}, restatement {a[bad[0], col]}"
    assert dev["cigars"].shape == cg.shape and (dev["cigars"] == cg).all(), "CIGAR words differ"


def slot_loop(shapes):
    """(passes, final cig_w) of the slot loop for these regions: slots of 16, 32, .. words hold two clips and the most operations any call leaves."""
    w, passes = 16, 1
    while int(shapes[:, 18].max()) > w - 2:
        w, passes = 2 * w, passes + 1
    return passes, w


def check_census(cen, flat, shapes, passes, cig_w, punts=True):
    """The stage's census against the counts the restatement's shape rows give, exactly."""
    want = census_from_shapes(flat, shapes)
    assert slot_loop(shapes) == (passes, cig_w), slot_loop(shapes)
    assert (cen["cig_w"], cen["passes"]) == (cig_w, passes), (cen["cig_w"], cen["passes"])
    assert cen["queued"] == int(want["queued"].sum()) and cen["big"] == int(want["big"].sum()), (cen["queued"], cen["big"])
    assert len(flat["rows"]) - cen["queued"] - cen["big"] == int(want["inline"].sum())
    assert cen["per_class"] == want["per_class"], (cen["per_class"], want["per_class"])
    rows = cen["rows"]
    assert sorted(rows[:, 0].tolist()) == np.flatnonzero(want["queued"]).tolist(), "the queue does not hold exactly the gapped regions"
    assert (rows[:, 1] == want["klass"][rows[:, 0]]).all(), "a queued region sits in another band class than its first n_col names"
    if punts:
        assert cen["punts"] == int(want["punt"].sum()), (cen["punts"], int(want["punt"].sum()))
    return want


def check_slices(cen, want):
    """Per queued region: the slice of traceback matrix it was given holds the rows of its widest executed try (hip_nw_coop.h: a row takes
    16 x max(the class's tiling, the smallest tiling that holds n_col) bytes)."""
    rows = cen["rows"]
    short = np.flatnonzero(rows[:, 2] * 64 < want["need_bytes"][rows[:, 0]])
    assert len(short) == 0, f"slice too small for region {rows[short[0], 0]}: {rows[short[0], 2] * 64} bytes < {want['need_bytes'][rows[short[0], 0]]}"


def reads_without_overflow(flat, shapes):
    """The reads none of whose regions needs more than a 16-word slot, by the restatement (no call leaves more than 14 operations: the
    stage checks the slot after every call, before squeeze and clips)."""
    over = set(int(r) for r in flat["read_of"][shapes[:, 18] > 14])
    return [i for i in range(len(flat["lens"])) if i not in over]


def subset(flat, exp, sub):
    """expected() of a sub-batch (flatten(b, reads)) cut from the whole batch's (CIGAR offsets renumbered)."""
    first = np.concatenate([[0], np.cumsum(flat["n_regs"])])
    g = np.concatenate([np.arange(first[i], first[i + 1]) for i in sub["ids"]] + [np.zeros(0, np.int64)]).astype(np.int64)
    a = exp["alns"][g].copy()
    cg = [exp["cigars"][exp["alns"][k, 8]:exp["alns"][k, 8] + exp["alns"][k, 7]] for k in g]
    a[:, 8] = np.concatenate([[0], np.cumsum(a[:, 7])[:-1]]) if len(g) else 0
    return dict(alns=a, cigars=np.concatenate(cg + [np.zeros(0, np.uint32)]).astype(np.uint32), shapes=exp["shapes"][g])


SLOT_CASES = (("core 14 with both clips", 1, 16), ("core 14 with lead D", 1, 16), ("core 15", 2, 32), ("core 30", 2, 32), ("core 31", 3, 64))


def slot_batches(b, flat, exp, only=None):
    """Each slot case's read on its own, both strands -> (tag, sub-batch, its expected(), passes, cig_w): 16 words exactly cost no retry, one
    operation more costs one, 32 words exactly stop at 32, one more reaches 64."""
    for tag, passes, cig_w in SLOT_CASES:
        if only is not None and tag != only:
            continue
        for sfx in "+-":
            i = next(k for k in range(len(b.reads)) if b.tags[k] and b.tags[k][0] == tag + sfx)
            sub = flatten(b, [i])
            sexp = subset(flat, exp, sub)
            assert slot_loop(sexp["shapes"]) == (passes, cig_w), (tag + sfx, slot_loop(sexp["shapes"]))
            yield tag + sfx, sub, sexp, passes, cig_w

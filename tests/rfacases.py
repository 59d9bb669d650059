"""Hand-planted inputs of the placement stage (arx_selftest_rfa, the restatement's ora_rfa): alignments on synthetic positions, no genome.

rows() is the helper of tests/test_rfa.py with several contigs and a contig per candidate.  build() makes ONE batch of many barcodes that sit on
the edges of rfa_barcode's workgroup code: candidate counts around the sort sizes and the lane count, both sides of the small-class rule,
surviving molecule counts around 64 and 1024 and one of 2049, contigs first seen out of index order, equal positions, unfiltered candidates,
moves whose winning sink has a high index, arg-max ties, neighbours exactly 50,000 and 50,001 apart, a barcode without RFA in the middle, a
centromere.  Every barcode carries what it
claims (`Barcode.claims`); tests/test_rfa_cases_hostsim.py holds the claims to the restatement's output before anything is compared with it.
Pure numpy; reads are 150 bases."""
import numpy as np

READ_LEN = 150
CONTIG_LEN = 250_000_000
N_SEQS = 4
ANN_OFF = [i * CONTIG_LEN for i in range(N_SEQS)]
L_PAC = N_SEQS * CONTIG_LEN               # only a number here: molecules can lie 60 kb apart by the thousand
CENTROMERES = ([0, 5_000_000, 0, 0], [0, 6_000_000, 0, 0])   # contig 1 alone; (0, 0] holds no position
GAP = 60_000                              # between two regions: more than the 50 kb that splits molecules, plus a pair's span


def rows(cands, l_pac=L_PAC, ann_off=(0,)):
    """cands: list per read of dicts(pos, rev, score, nm, cigar=[(op,len)...], rid=0) -> oracle input rows; pos is contig-relative.
    A reverse-strand candidate with leftmost position P covers [P, P+150): aligner.go:1577-1582 with gobwa.go:351-363."""
    reg_off, regs, alns, cig = [0], [], [], []
    for read in cands:
        for c in read:
            rid = c.get("rid", 0)
            off = ann_off[rid]
            if c["rev"]:
                cend = c["pos"] - 1 + off      # pos = Alignment_end + 1
                re_ = 2 * l_pac - 1 - cend
                rb = re_ - READ_LEN
            else:
                rb, re_ = c["pos"] + off, c["pos"] + off + READ_LEN
            r = [0] * 20
            r[0], r[1], r[2], r[3], r[4], r[5], r[6] = rb, re_, 0, READ_LEN, rid, c["score"], c["score"]
            regs.append(r)
            cg = c.get("cigar", [(0, READ_LEN)])
            alns.append([0, rid, 0, int(c["rev"]), 0, 0, c.get("nm", 0), len(cg), len(cig), c["score"], 0, 0])
            cig += [(ln << 4) | op for op, ln in cg]
        reg_off.append(len(regs))
    return dict(reg_off=np.array(reg_off), regs=np.array(regs, dtype=np.int64).reshape(-1, 20), alns=np.array(alns, dtype=np.int64).reshape(-1, 12),
                cigars=np.array(cig + [0], dtype=np.uint32))


def fwd(pos, rid=0, score=150, **kw):
    return dict(pos=pos, rev=False, score=score, rid=rid, **kw)


def rev(pos, rid=0, score=150, **kw):
    return dict(pos=pos, rev=True, score=score, rid=rid, **kw)


class Barcode:
    """One barcode under construction.  Regions come from an allocator that keeps them more than 50 kb apart on a contig, in ascending order, so
    a region is a molecule and the molecules of a contig are numbered in allocation order (contigs in first-seen order)."""

    def __init__(self, name, do_rfa=True, start=None):
        self.name, self.do_rfa, self.reads = name, do_rfa, []
        self.cur = dict(start or {})
        self.n_live = 0          # regions that hold an alignment tagBestAlignments makes active: the molecules that survive scrapMolecules
        self.placeholder = False
        self.claims = dict(movers=[], ties=[])   # movers: (pair, listing index the reads end on, smallest index the winning sink may have)

    def region(self, rid, span, live=True):
        s = self.cur.get(rid, 1_000_000)
        self.cur[rid] = s + span + GAP
        self.n_live += 1 if live else 0
        return s

    def pair(self, f, r):
        self.reads += [f, r]
        if not f or not r:
            self.placeholder = True
        return len(self.reads) // 2 - 1

    @property
    def n_c(self):
        return sum(max(1, len(r)) for r in self.reads)

    @property
    def n_mol(self):
        return self.n_live + (1 if self.placeholder else 0)   # every read without hits lies at position -1 of contig "": one molecule

    # ---- building blocks
    def iso(self, rid=0):
        s = self.region(rid, 200)
        return self.pair([fwd(s, rid)], [rev(s + 200, rid)])

    def dense(self, rid, n_pairs, span=None):
        """n_pairs unique pairs 700 apart: one molecule (active from five reads on).  Returns its start."""
        s = self.region(rid, span if span else n_pairs * 700 + 200)
        for i in range(n_pairs):
            self.pair([fwd(s + i * 700, rid)], [rev(s + i * 700 + 200, rid)])
        return s

    def mover(self, sinks, lone_rid=0, min_sink=0, expect=None, tie=None):
        """A pair whose first-listed placement lies alone and whose others lie inside dense molecules (sinks: (start, rid, offset)).  tagBestAlignments
        keeps the first (exact tie: first pair wins); fastScore(lone -> dense) = +3 (the source empties), so the sweep moves both reads."""
        s = self.region(lone_rid, 200)
        f, r = [fwd(s, lone_rid)], [rev(s + 200, lone_rid)]
        for start, rid, o in sinks:
            f.append(fwd(start + o, rid)); r.append(rev(start + o + 200, rid))
        p = self.pair(f, r)
        self.claims["movers"].append((p, len(sinks) if expect is None else expect, min_sink))
        if tie:
            self.claims["ties"].append((p, len(sinks) if expect is None else expect, tie))
        return p

    def unit(self, rid, lone_rid, lone_first):
        """33 candidates: a dense molecule of six pairs with, inside it, the second placement of a lone pair, a pair with an unfiltered extra, a pair at
        the positions of another, a read with two identical placements, a read whose second-listed placement lies left of its first; and a pair
        with three equal placements in regions of their own (two of them hold nothing active and disappear)."""
        lone = None
        if lone_first:       # the lone region in front of the dense one: a smaller molecule index than its sink's
            lone = self.region(lone_rid, 200)
        s = self.dense(rid, 6, span=6000)
        if lone is None:
            lone = self.region(lone_rid, 200)
        p = self.pair([fwd(lone, lone_rid), fwd(s + 250, rid)], [rev(lone + 200, lone_rid), rev(s + 450, rid)])
        self.claims["movers"].append((p, 1, 0))
        self.pair([fwd(s + 950, rid), fwd(s + 1000, rid, score=100)], [rev(s + 1150, rid)])            # 100 < 150 - 17: outside the RFA lists
        self.pair([fwd(s, rid)], [rev(s + 200, rid)])                                                    # equal positions, other reads: candidate index decides
        self.pair([fwd(s + 1650, rid), fwd(s + 1650, rid)], [rev(s + 1850, rid)])                        # equal positions, one read: the first keeps the spot
        self.pair([fwd(s + 2400, rid), fwd(s + 2100, rid)], [rev(s + 2500, rid)])                        # equal scores: the smaller position takes the spot
        far = [self.region(lone_rid, 200, live=(i == 0)) for i in range(3)]
        self.pair([fwd(x, lone_rid) for x in far], [rev(x + 200, lone_rid) for x in far])
        return s

    def fill_to(self, n_c, order=(2, 0, 3, 1)):
        """Units while they fit, then one pair with a read without hits where the count is odd, then unique pairs in one molecule."""
        u = 0
        while n_c - self.n_c >= 33 + 3:
            # even units: the lone pair in front of its sink on the sink's contig (unit 0: molecule 0 of the barcode); odd units: behind it, on the next contig
            self.unit(order[u % 4], order[u % 4] if u % 2 == 0 else order[(u + 1) % 4], lone_first=(u % 2 == 0))
            u += 1
        left = n_c - self.n_c
        assert left >= 0
        if left & 1:
            a, b = self.region(order[0], 200), self.region(order[0], 200, live=False)
            self.pair([], [rev(a, order[0]), rev(b, order[0])])
            left -= 3
        assert left >= 0 and left % 2 == 0
        if left:
            self.dense(order[1], left // 2)
        assert self.n_c == n_c, (self.name, self.n_c, n_c)
        return self


def edge_barcode(n_c):
    b = Barcode(f"n_c={n_c}")
    if n_c == 2:
        b.iso()
        return b
    return b.fill_to(n_c)


def molecules_barcode(n_mol):
    """n_mol surviving molecules: isolated pairs; from 65 on with a dense molecule behind all of them that a lone pair moves into, so the winning sink's
    index is n_mol - 1 >= 64 (>= 1024 in the barcodes of 1025 and 2049)."""
    b = Barcode(f"molecules={n_mol}")
    if n_mol in (65, 1025):
        for _ in range(n_mol - 2):
            b.iso()
        lone_p = len(b.reads) // 2
        d = None
        lone = b.region(0, 200)
        d = b.dense(0, 6, span=6000)
        p = b.pair([fwd(lone), fwd(d + 250)], [rev(lone + 200), rev(d + 450)])
        assert p >= lone_p
        b.claims["movers"].append((p, 1, n_mol - 1))
    elif n_mol > 2000:
        # 2049 = 2040 isolated + three dense (A at index 500, B at 1601, C last) + six lone pairs: five move into C (index 2048), one has equally good
        # placements in B and in A, listed in that order: the arg-max meets A in a lane's first stride and B in another lane's second, A wins
        for _ in range(500):
            b.iso()
        a = b.dense(0, 6, span=6000)
        for _ in range(1100):
            b.iso()
        bb = b.dense(0, 6, span=6000)
        for _ in range(n_mol - 9 - 1600):
            b.iso()
        lones = [b.region(0, 200) for _ in range(6)]
        c = b.dense(0, 6, span=6000)
        for i, lone in enumerate(lones[:5]):
            p = b.pair([fwd(lone), fwd(c + 250 + 10 * i)], [rev(lone + 200), rev(c + 450 + 10 * i)])
            b.claims["movers"].append((p, 1, 1024))
        lone = lones[5]
        p = b.pair([fwd(lone), fwd(bb + 250), fwd(a + 250)], [rev(lone + 200), rev(bb + 450), rev(a + 450)])
        b.claims["movers"].append((p, 2, 500))
        b.claims["ties"].append((p, 2, "equal sinks at indices 500 and 1601: the smaller wins"))
    else:
        for _ in range(n_mol):
            b.iso()
    if n_mol >= 1023:      # a large barcode: one placement below best - 17 in it (outside the RFA lists, in no molecule)
        b.reads[0].append(fwd(b.reads[0][0]["pos"] + 30, score=100))
    assert b.n_mol == n_mol, (b.n_mol, n_mol)
    return b


def neighbours_barcode():
    """inferMolecules splits where two neighbours in position order lie MORE than 50,000 apart: pair A, then pair B whose forward read starts exactly
    50,000 behind A's reverse read (one molecule with A), then pair C exactly 50,001 behind B's reverse read (a molecule of its own); the same again
    on contig 2 behind a dense molecule.  Every pair is unique, so each side keeps its active alignments and both molecules survive."""
    b = Barcode("neighbours")
    b.claims["neighbours"] = []
    for rid, lead in ((0, 0), (2, 6)):
        if lead:
            b.dense(rid, lead, span=6000)
        s = b.region(rid, 200 + 50_000 + 200 + 50_001 + 200)      # two molecules in this stretch: one more than region() counted
        b.n_live += 1
        pb, pc = s + 200 + 50_000, s + 200 + 50_000 + 200 + 50_001
        trio = tuple(b.pair([fwd(x, rid)], [rev(x + 200, rid)]) for x in (s, pb, pc))
        b.claims["neighbours"].append(trio)
    return b


def ties_barcode():
    """Two equally good sinks of equal size in different waves (indices 1 and 73, the larger listed first), and two that differ in their active
    alignments alone (indices 2 and 74, the smaller molecule listed last but one): the key's low word decides for the larger one."""
    b = Barcode("ties")
    b.iso()
    a = b.dense(0, 6, span=6000)          # index 1
    d = b.dense(0, 6, span=6000)          # index 2: 12 active alignments
    for _ in range(70):
        b.iso()                           # 3 .. 72
    bb = b.dense(0, 6, span=6000)         # index 73
    e = b.dense(0, 7, span=6000)          # index 74: 14 active alignments
    b.mover([(bb, 0, 250), (a, 0, 250)], expect=2, min_sink=1, tie="equal sinks at indices 1 and 73: the smaller wins")
    b.mover([(d, 0, 250), (e, 0, 250)], expect=2, min_sink=74, tie="sinks equal but for 12 against 14 active alignments: the larger molecule wins")
    b.claims["sink_index"] = {0: 1, 1: 74}
    return b


def contigs_barcode(nohit_first):
    """Contigs first seen in the order 3, 0, 1, 2 -- or "", 2, 3, 0, 1 where a read without hits is listed first (contig -1); the molecules on contig 1 lie
    in its centromere; a lone pair on contig 3 (molecule index 0 when no read without hits comes first) moves into the dense molecule on contig 0."""
    b = Barcode("contigs, read without hits first" if nohit_first else "contigs", start={1: 5_400_000})
    if nohit_first:
        s = b.region(2, 200)
        b.pair([], [rev(s, 2)])
    lone = b.region(3, 200)
    first = len(b.reads) // 2
    b.reads += [None, None]               # the mover is listed first of the pairs with hits: its contig is seen first
    for rid in (1, 2, 0):
        b.dense(rid, 6, span=6000)
    d0 = b.cur[0] - 6000 - GAP
    b.reads[2 * first], b.reads[2 * first + 1] = [fwd(lone, 3), fwd(d0 + 250, 0)], [rev(lone + 200, 3), rev(d0 + 450, 0)]
    b.claims["movers"].append((first, 1, 0))
    b.dense(3, 6, span=6000)
    b.dense(1, 5)
    return b


def small_rule_barcodes():
    out = [Barcode("256 pairs x 1 candidate"), Barcode("257 pairs x 1 candidate"), Barcode("200 pairs, 513 candidates")]
    out[0].dense(0, 256)
    out[1].dense(0, 257)
    s = out[2].dense(0, 87)
    for i in range(113):
        p = s + 700 * (87 + i)
        out[2].pair([fwd(p), fwd(p + 30, score=100)], [rev(p + 200)])
    out[2].cur[0] += 700 * 113
    assert (out[0].n_c, out[1].n_c, out[2].n_c) == (512, 514, 513) and len(out[2].reads) == 400
    return out


EDGE_N_C = (2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048, 2049, 4095, 4096, 4097, 6003)
MOLECULES = (63, 64, 65, 1023, 1024, 1025, 2049)


def build():
    """-> dict(barcodes, rows, lens, bc_pair_off, do_rfa, n_reads): one batch, the barcode without RFA in the middle."""
    bcs = [edge_barcode(n) for n in EDGE_N_C[:8]] + small_rule_barcodes() + [molecules_barcode(n) for n in MOLECULES[:4]]
    off = Barcode("no RFA", do_rfa=False).fill_to(100)
    bcs += [ties_barcode(), off, contigs_barcode(False), contigs_barcode(True), neighbours_barcode()]
    bcs += [molecules_barcode(n) for n in MOLECULES[4:]] + [edge_barcode(n) for n in EDGE_N_C[8:]]
    reads, po = [], [0]
    for b in bcs:
        reads += b.reads
        po.append(len(reads) // 2)
    return dict(barcodes=bcs, rows=rows(reads, L_PAC, ANN_OFF), lens=np.full(len(reads), READ_LEN, dtype=np.int32), bc_pair_off=np.array(po, dtype=np.int64),
                do_rfa=np.array([b.do_rfa for b in bcs], dtype=np.uint8), n_reads=len(reads))


def small_class_rule(case):
    """pipeline_rfa.h: at most 2 * SMALL_LANES reads and at most SMALL_SORT / 2 candidates."""
    return np.array([len(b.reads) <= 512 and b.n_c <= 512 for b in case["barcodes"]], dtype=np.uint8)


def oracle(case, do_rfa=None):
    """The restatement on the batch (do_rfa: other flags than the batch's own)."""
    import rfadrv
    return rfadrv.oracle_rfa(case["rows"], case["lens"], case["bc_pair_off"], case["do_rfa"] if do_rfa is None else do_rfa, L_PAC, ANN_OFF, centromeres=CENTROMERES)


def run_device(case, lib_path, **kw):
    from arachne_amd import api
    return api.selftest_rfa(case["rows"], case["lens"], case["bc_pair_off"], case["do_rfa"], L_PAC, ANN_OFF, centromeres=CENTROMERES, lib_path=lib_path, **kw)


def check_device(case, dev, small_expected):
    """dev: api.selftest_rfa's result against case["ora"]: every candidate field (parity.check_rfa), the molecule count per barcode, the class bytes."""
    import parity
    parity.check_rfa(dev, case["ora"])
    rows, po, off = case["ora"]["cands"], case["bc_pair_off"], case["ora"]["cand_off"]
    for i, b in enumerate(case["barcodes"]):
        lo, hi = int(off[2 * po[i]]), int(off[2 * po[i + 1]])
        assert dev["barcodes"]["n_mol"][i] == (int(rows[lo:hi, 15].max()) + 1 if b.do_rfa else 0), b.name
    assert (dev["cls"] == small_expected).all(), (dev["cls"], small_expected)
    assert (dev["cands"]["active"] == 1).sum() == case["n_reads"]

"""Seeded test workloads shared by the golden generator and the parity tests."""
import os
import tempfile

import numpy as np

from arachne_amd import synth

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def nasty_genome(seed, contig_lens=(60000, 30000, 10000), alt_contigs=1):
    """Repeat-rich genome: interspersed families, exact copies, tandem repeats, a homopolymer, N runs."""
    rng = np.random.default_rng(seed)
    g = synth.make_genome(100 + seed, list(contig_lens),
                          repeat_families=[(40, 300, 0.08), (12, 2000, 0.03), (4, 6000, 0.01), (20, 150, 0.0)],
                          alt_contigs=alt_contigs)
    for ci in range(len(contig_lens)):
        s = g.seqs[ci]
        for _ in range(5):
            unit = rng.integers(0, 4, size=int(rng.integers(2, 60)), dtype=np.uint8)
            n = int(rng.integers(5, 40))
            if len(unit) * n + 2 >= len(s):
                continue
            p = int(rng.integers(0, len(s) - len(unit) * n - 1))
            tr = synth._mutate(rng, np.tile(unit, n), 0.02)
            s[p:p + len(tr)] = tr
        p = int(rng.integers(0, len(s) - 300))
        s[p:p + 200] = 0
    return g


def nasty_reads(seed, g, n_barcodes=4, pairs_per_barcode=150):
    """High-error pairs plus corrupted mates (forces rescue), random reads, N runs, chimeras, big indels."""
    rng = np.random.default_rng(1000 + seed)
    rs = synth.make_reads(200 + seed, g, n_barcodes, pairs_per_barcode, sub_rate=0.02, indel_rate=0.004,
                          molecule_len=20000, molecules_per_barcode=3)
    S = rs.seqs
    n = S.shape[0]
    for i in rng.choice(n, size=n // 5, replace=False):
        m = rng.random(150) < 0.12
        S[i, m] = rng.integers(0, 4, size=int(m.sum()), dtype=np.uint8)
    for i in rng.choice(n, size=max(1, n // 50), replace=False):
        S[i] = rng.integers(0, 4, size=150, dtype=np.uint8)
    for i in rng.choice(n, size=max(1, n // 30), replace=False):
        p = int(rng.integers(0, 140))
        S[i, p:p + int(rng.integers(1, 12))] = 4
    for i in rng.choice(n, size=max(1, n // 30), replace=False):
        j = int(rng.integers(0, n))
        p = int(rng.integers(30, 120))
        S[i, p:] = S[j, p:]
    for i in rng.choice(n, size=max(1, n // 40), replace=False):
        p = int(rng.integers(30, 100))
        L = int(rng.integers(5, 40))
        S[i, p:150 - L] = S[i, p + L:].copy()
    return rs


INDEX_EXTS = ("bwt", "sa", "pac", "ann", "amb", "alt")


def pack_index(prefix):
    """Index files -> dict of uint8 arrays (stored inside the golden .npz)."""
    out = {}
    for ext in INDEX_EXTS:
        fn = prefix + "." + ext
        if os.path.exists(fn):
            out["idx_" + ext] = np.fromfile(fn, dtype=np.uint8)
    return out


def unpack_index(npz, dirname, name="golden.fa"):
    prefix = os.path.join(dirname, name)
    for ext in INDEX_EXTS:
        key = "idx_" + ext
        if key in npz:
            np.asarray(npz[key], dtype=np.uint8).tofile(prefix + "." + ext)
    return prefix


def long_reads(read_len, n_bc=3, ppb=300, mixed=False, contig=1_200_000):
    """Pairs of the given length (up to MAX_READ_LEN = 255), a quarter of the reads corrupted (15 % or 35 % of their bases) so that the rescue SW has work; mixed: every
    third pair keeps only its first 150 bases (a batch that holds both element sizes of ksw_align2: KSW_XBYTE below 250 bases, ksw_i16
    from there on, bwamem_pair.c:150).  Returns genome, ReadSet, sequences (2-D, or flat when mixed) and lengths."""
    from arachne_amd import synth
    g = synth.make_genome(500 + read_len, [contig])
    rs = synth.make_reads(501 + read_len, g, n_bc, ppb, read_len=read_len, sub_rate=0.01)
    rng = np.random.default_rng(read_len)
    for i in rng.choice(rs.seqs.shape[0], size=rs.seqs.shape[0] // 4, replace=False):
        m = rng.random(read_len) < (0.15, 0.35)[i & 1]
        rs.seqs[i, m] = rng.integers(0, 4, size=int(m.sum()), dtype=np.uint8)
    seqs, lens = rs.seqs, rs.lens
    if mixed:
        lens = lens.copy()
        lens[4::6] = 150
        lens[5::6] = 150
        seqs = np.concatenate([rs.seqs[r, :lens[r]] for r in range(len(lens))])
    return g, rs, seqs, lens


def _rc(a):
    a = np.asarray(a, dtype=np.uint8)[::-1]
    return np.where(a > 3, 4, 3 - a).astype(np.uint8)


def _plant_two_sided(rng, s, pos, ml, fl, step, stride=1500):
    """Copies of a master (ml bases) that equal it up to depth d (d = 16, 16 + step, ...), differ at d and are random behind; each copy carries
    the last e bases of a flank F (fl bases) in front of it, the base before them forced to differ.  Then F once in full, followed by a base
    that is not master[0].  A read F + master[:L] dies at |F| in its first forward extension; the next start is the master's first base with F to
    its left: a long forward list whose backward sweep stays wide for many rows.  Returns (master, F, end position)."""
    master = rng.integers(0, 4, size=ml, dtype=np.uint8)
    F = rng.integers(0, 4, size=fl, dtype=np.uint8)
    for d in range(16, ml - 2, step):
        c = master.copy()
        c[d] = (c[d] + 1 + (d >> 1) % 3) % 4
        c[d + 1:] = rng.integers(0, 4, size=ml - d - 1, dtype=np.uint8)
        e = 1 + (d * 7) % (fl - 6)
        s[pos - e:pos] = F[fl - e:]
        s[pos - e - 1] = (F[fl - e - 1] + 1) % 4
        s[pos:pos + ml] = c
        pos += stride
    s[pos:pos + fl] = F
    s[pos + fl] = (master[0] + 2) % 4
    return master, F, pos + stride


def seed_shapes(seed=7, cap=255, nasty_pairs=300):
    """Genome and reads that take the seeding kernels through their rare paths (tests/test_seed_shapes_hostsim.py asserts from the
    restatement that they do; tests/test_seed_variants_gpu.py runs every kernel variant on them).
      * forward-graded family: ~120 copies of a 255-base master that equal it up to graded depths; reads = its prefixes and the suffixes of its
        reverse complement: first-pass forward lists of every length up to ~130 (list buffers, pool slices, the owed prefix, text mode late);
      * two two-sided families (_plant_two_sided; flank 55 / master 200 / every other depth, and flank 20 / master 235 / every depth): long lists
        whose start lies inside the read, swept backwards for tens of rows (deep) or more than 200 entries wide (wide);
      * exact copies: a 100-base unit 600 times (above max_occ), a 120-base unit 30 times, 150-base units 2 .. 25 times (around split_width = 10 and
        max_mem_intv = 20); reads inside them, across their ends with 0 .. 23 unique bases behind, with a planted difference;
      * the first and last 300 bases of every contig on both strands, ambiguous bases at the positions the table jumps look at, reads of 18-20 bases;
      * a slice of the nasty reads for ordinary traffic.
    Reads are shuffled; lengths 18 .. 255, or cut to their first `cap` bases.  Returns (genome, flat bases, lens, dict of read index arrays by kind)."""
    rng = np.random.default_rng(seed)
    g = nasty_genome(seed, contig_lens=(600000, 800000, 120000, 50000), alt_contigs=1)
    s0, s1, s2, s3 = g.seqs[0], g.seqs[1], g.seqs[2], g.seqs[3]
    reads, kind = [], []

    def add(k, r):
        r = np.asarray(r, dtype=np.uint8)
        if len(r) >= 1:
            reads.append(r[:255].copy())
            kind.append(k)

    # forward-graded family (contig 0, 1000 .. 181000)
    ML = 255
    master = rng.integers(0, 4, size=ML, dtype=np.uint8)
    pos = 1000
    for d in range(16, ML - 2, 2):
        c = master.copy()
        c[d] = (c[d] + 1 + (d >> 1) % 3) % 4
        c[d + 1:] = rng.integers(0, 4, size=ML - d - 1, dtype=np.uint8)
        s0[pos:pos + ML] = c
        pos += 1500
    s0[pos:pos + ML] = master
    for L in range(19, ML + 1):
        add("graded", master[:L])
    rcm = _rc(master)
    for L in range(19, ML + 1, 3):
        add("graded", rcm[ML - L:])
    # exact copies (contig 0, 250000 .. 550000: the 600-fold unit; contig 3: the 30-fold one; contig 2: 2 .. 25 copies)
    unit600 = rng.integers(0, 4, size=100, dtype=np.uint8)
    at600 = [250000 + 500 * j for j in range(600)]
    for p in at600:
        s0[p:p + 100] = unit600
    unit30 = rng.integers(0, 4, size=120, dtype=np.uint8)
    at30 = [2000 + 1200 * j for j in range(30)]
    for p in at30:
        s3[p:p + 120] = unit30
    few = []
    p = 5000
    for copies in (2, 3, 5, 8, 9, 10, 11, 12, 15, 19, 20, 21, 25):
        u = rng.integers(0, 4, size=150, dtype=np.uint8)
        at = []
        for _ in range(copies):
            s2[p:p + 150] = u
            at.append(p)
            p += 400
        few.append((u, at))
    for j in (0, 7, 299, 599):
        cp = at600[j]
        for t in range(0, 24):                      # the unit, then t unique bases: the unique stretch begins within the last t bases of the read
            add("copies", s0[cp:cp + 100 + t])
            add("copies", _rc(s0[cp - t:cp + 100]))
        add("copies", s0[cp - 60:cp + 160])
        add("copies", s0[cp + 10:cp + 90])
        r = s0[cp - 30:cp + 130].copy()
        r[80] = (r[80] + 1) % 4
        add("copies", r)
    for j in (0, 13, 29):
        cp = at30[j]
        for t in (0, 1, 5, 9, 10, 11, 14, 15, 19, 20, 40):
            add("copies", s3[cp:cp + 120 + t])
        add("copies", s3[cp - 50:cp + 170])
        add("copies", _rc(s3[cp - 20:cp + 120]))
    for u, at in few:
        for cp in (at[0], at[-1]):
            add("copies", s2[cp:cp + 150])
            add("copies", s2[cp - 40:cp + 190])
            add("copies", _rc(s2[cp - 10:cp + 150]))
            add("copies", s2[cp + 20:cp + 120])
            r = s2[cp - 20:cp + 170].copy()
            r[95] = (r[95] + 2) % 4
            add("copies", r)
    # the two two-sided families (contig 1)
    mA, FA, end = _plant_two_sided(rng, s1, 1000, 200, 55, 2)
    mB, FB, end = _plant_two_sided(rng, s1, end + 1000, 235, 20, 1)
    assert end < len(s1) - 1000
    for L in range(21, 201):
        add("two_sided", np.concatenate([FA, mA[:L]]))
    for L in range(22, 236):
        add("two_sided", np.concatenate([FB, mB[:L]]))
    # the ends of every contig (and with them of the whole text, forward and reverse complement, and the seam between the two at l_pac)
    for s in g.seqs:
        n = len(s)
        for o, L in ((0, 150), (0, 255), (0, 19), (1, 100), (2, 64), (3, 65), (5, 128), (17, 200), (45, 255), (64, 150), (100, 200), (149, 151)):
            add("edges", s[o:o + L])
            add("edges", _rc(s[o:o + L]))
            add("edges", s[n - o - L:n - o])
            add("edges", _rc(s[n - o - L:n - o]))
    # ambiguous bases where the table jumps look (the first K bases of a start, the 19 bases the third pass jumps over, right behind them; K = 4 .. 15),
    # at the front of the read and in front of its end; reads of 18, 19, 20 bases
    base = [s1[600000:600150], s2[60000:60150], s0[at600[300] - 20:at600[300] + 130]]
    for b in base:
        for p in (0, 1, 3, 4, 5, 9, 10, 11, 13, 14, 15, 16, 18, 19, 20, 21, 40):
            r = b.copy()
            r[p] = 4
            add("edges", r)
            r = b.copy()
            r[len(r) - 1 - p] = 4
            add("edges", r)
            r = b.copy()
            r[60] = 4
            r[60 + 1 + p] = 4
            add("edges", r)
        for L in (18, 19, 20):
            add("edges", b[:L])
            add("edges", _rc(b[50:50 + L]))
    # ordinary traffic
    rs = nasty_reads(seed, g, n_barcodes=2, pairs_per_barcode=nasty_pairs // 2)
    for r in range(rs.seqs.shape[0]):
        add("nasty", rs.seqs[r, :rs.lens[r]])
    if len(reads) & 1:
        add("edges", s1[700000:700150])
    order = rng.permutation(len(reads))
    reads = [reads[i][:cap] for i in order]
    kind = [kind[i] for i in order]
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    kinds = {k: np.nonzero(np.array(kind) == k)[0] for k in ("graded", "two_sided", "copies", "edges", "nasty")}
    flat = np.concatenate(reads)
    assert flat.max() <= 4
    return g, flat, lens, kinds


def _other(*bases):
    """A base (0 .. 3) that equals none of the given ones (at most three distinct)."""
    for b in range(4):
        if b not in [int(x) for x in bases]:
            return b
    raise ValueError("no base left")


# the exact-copy families of list_shapes: a read piece of LIST_S_LEN[a] / LIST_P_LEN[c] bases has exactly 20 * a / c occurrences
LIST_S_MAX, LIST_E_COPIES, LIST_E_LEN, LIST_U_LEN = 25, 400, 61, 60
LIST_S_LEN = {a: 87 - a for a in range(1, LIST_S_MAX + 1)}      # a = 1 .. 25: 86 .. 62 bases, 20 .. 500 occurrences
LIST_P_LEN = {c: 102 - c for c in range(20, 41)}                # c = 20 .. 40: 82 .. 62 bases


def list_shapes(seed=11, nasty_pairs=60):
    """Genome and read PAIRS that take the wavefront-per-item list kernels (k_chain_heavy, k_dedup_heavy, k_rescue_heavy) to their lane, word
    and LDS-class edges (tests/test_list_shapes_hostsim.py asserts from the restatement that they do; tests/test_wave_lists_gpu.py runs every
    kernel variant on them).  Every planted copy has the bases next to it forced to differ from what a read has there, so that the counts
    are exact.
      * contig 0, exact-copy families at a stride of 120 bases.  S: the last 62 .. 86 bases of a master, 20 copies per length -- a read piece
        of the last LIST_S_LEN[a] bases occurs 20 * a times (a = 1 .. 25).  E: a 61-mer 400 times.  P: the first 62 .. 82 bases of a master,
        20 copies of all 82 and one per shorter length -- the first LIST_P_LEN[c] bases occur c times (c = 20 .. 40).  A read S + E + P has
        20 a + 400 b + c seed occurrences, one chain and one region each.  U: a 60-mer planted once and its bases 20 .. 40 once more elsewhere:
        between pieces with NX occurrences (all longer than 60; the read is S + U + E + P) the 20-base chain is dropped by the chain of kept
        rank NX.  Behind them two families of 66 loci whose reads seed far off the diagonal inside their own alignment (see there): regions
        the read's own de-duplication pass finds redundant, the earlier or the later of the two going;
      * contig 1, pair families at a stride of 420: read 1 (100 bases) exact in all loci but the d that come first in read 2's list, where
        every 8th base differs (no seed: the region is rescued and inserted at the end of read 1's list while it grows from loci - d);
        "first": read 1's first 45 bases exact everywhere, the rest random, but for three loci that hold all of it with every 16th base
        changed (rescued with a higher score than any listed region: inserted at position 0); "far": both reads exact everywhere, the
        pairs 506 .. 580 bases long -- listed, but no proper pair, so the rescue finds the listed region again (ties) or a part of it
        (a redundant entry for the pass to remove).  Every family gives two pairs, the second with the reads swapped (the second rescue loop);
      * a slice of the nasty reads (contig 2 and an ALT contig) for ordinary traffic.
    Returns (genome, flat bases, lens, dict of read index arrays by kind); reads 2i and 2i + 1 are a pair."""
    rng = np.random.default_rng(seed)
    g = nasty_genome(seed, contig_lens=(180000, 390000, 30000), alt_contigs=1)
    s0, s1 = g.seqs[0], g.seqs[1]
    s0[:] = rng.integers(0, 4, size=len(s0), dtype=np.uint8)      # (no ambiguous runs, families or tandems of the background inside the planted contigs)
    s1[:] = rng.integers(0, 4, size=len(s1), dtype=np.uint8)
    pairs, kind = [], []

    def add(k, r1, r2):
        pairs.append((np.asarray(r1, dtype=np.uint8).copy(), np.asarray(r2, dtype=np.uint8).copy()))
        kind.append(k)

    # ---- contig 0: S, E, P, U
    mS = rng.integers(0, 4, size=LIST_S_LEN[1], dtype=np.uint8)
    mE = rng.integers(0, 4, size=LIST_E_LEN, dtype=np.uint8)
    mP = rng.integers(0, 4, size=LIST_P_LEN[20], dtype=np.uint8)
    U = rng.integers(0, 4, size=LIST_U_LEN, dtype=np.uint8)
    # a read is S + U + E + P (any of them left out): whatever follows a piece begins with mE[0], whatever precedes one ends with mS[-1]
    mP[0] = U[0] = mE[0]
    mE[-1] = U[-1] = mS[-1]
    pos = [1000]

    def plant(body, before, after):
        p = pos[0]
        s0[p - 1] = before
        s0[p:p + len(body)] = body
        s0[p + len(body)] = after
        pos[0] = p + 120
        return p

    for a in range(1, LIST_S_MAX + 1):
        L = LIST_S_LEN[a]
        for _ in range(20):
            plant(mS[len(mS) - L:], _other(mS[len(mS) - L - 1]) if L < len(mS) else int(rng.integers(0, 4)), _other(mE[0]))
    for _ in range(LIST_E_COPIES):
        plant(mE, _other(mS[-1]), _other(mE[0]))
    for c in range(20, 41):
        L = LIST_P_LEN[c]
        for _ in range(20 if c == 20 else 1):
            plant(mP[:L], _other(mS[-1]), _other(mP[L]) if L < len(mP) else int(rng.integers(0, 4)))
    plant(U, _other(mS[-1]), _other(mE[0]))
    plant(U[20:40], _other(U[19]), _other(U[40]))
    assert pos[0] < len(s0) - 1000

    def chain_read(t, u=False):
        """A read with t = 20 a + 400 b + c seed occurrences (and U's two)."""
        b = 0
        if t == 400 or t > 539:
            b, t = 1, t - 400
        a, c = (0, t) if t <= 40 else ((t - 20 - t % 20) // 20, 20 + t % 20)
        assert 0 <= a <= LIST_S_MAX and (c == 0 or 20 <= c <= 40), (t, a, b, c)
        parts = [mS[len(mS) - LIST_S_LEN[a]:]] if a else []
        if u:
            parts.append(U)
        if b:
            parts.append(mE)
        if c:
            parts.append(mP[:LIST_P_LEN[c]])
        r = np.concatenate(parts)
        assert len(r) <= 255
        return r

    for t in (31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 831, 832, 833, 900, 939):
        r, other = chain_read(t), chain_read(20 + t % 21)
        add("chain", r, other)
        add("chain", _rc(other), _rc(r))
    # pairs by the sum of their core lists (the heavy threshold 47 | 48) and of their capacities (KPairCap: n0 + 2 n1 + 52 with n1 < 50 <= n0 + n1,
    # n0 + n1 + 102 from 50 regions each; the LDS classes 170 | 171, 340 | 341, 680 | 681)
    for t1, t2 in ((23, 24), (24, 24), (70, 24), (71, 24), (119, 119), (119, 120), (289, 289), (289, 290)):
        r1, r2 = chain_read(t1), chain_read(t2)
        add("cap", r1, r2)
        add("cap", _rc(r1), _rc(r2))
    # the kept rank of the chain that drops U's 20-base chain: the number of occurrences of the longer pieces around U
    for nx in (62, 63, 64, 65, 129, 400):
        r = chain_read(nx, u=True)
        add("rank", r, chain_read(25))
        add("rank", _rc(chain_read(26)), _rc(r))
    # ---- contig 0, behind them: regions the read's own de-duplication pass finds redundant (a seed inside an alignment's span but far off its
    # diagonal is extended on its own, mem_chain2aln's containment test, bwamem.c:683-699; between seeds on one diagonal nothing is)
    p0 = pos[0] + 1000
    X = rng.integers(0, 4, size=40, dtype=np.uint8)        # one copy in front of both families: an odd number of regions before the pairs
    # "redun_c": read = A (120) + A[5:25] + one base + B (60), locus = A + 20 other bases + another base + B.  The repeated 20 bases seed at the
    # locus's base 5, 115 off the diagonal: a 20-base region inside the long one, listed before it (its end comes first) and dropped by it
    A = rng.integers(0, 4, size=120, dtype=np.uint8)
    B = rng.integers(0, 4, size=60, dtype=np.uint8)
    first_e = int(rng.integers(0, 4))
    C = A[5:25].copy()
    A[119] = _other(A[4])
    sep = _other(A[25])
    Z = rng.integers(0, 4, size=20, dtype=np.uint8)
    Z[0], Z[10] = _other(C[0], A[119]), _other(C[10])
    s0[p0:p0 + 40] = X
    s0[p0 + 40] = _other(A[0], first_e)         # (not what follows X in a read)
    p0 += 400
    locus = np.concatenate([A, Z, [_other(sep)], B])
    for j in range(66):
        s0[p0 - 1] = _other(X[-1])
        s0[p0:p0 + len(locus)] = locus
        p0 += 450
    rc_ = np.concatenate([A, C, [sep], B])
    for r in (rc_, np.concatenate([X, rc_])):
        add("redun", r, chain_read(27))
        add("redun", _rc(chain_read(28)), _rc(r))
    # "redun_e": the read follows a 160-base locus with single differences that leave two 25-base seeds, and holds the locus's last 20 bases
    # and the base behind them once more at 19 .. 40 (where the locus has them with three differences).  Those 21 bases seed 121 off the
    # diagonal: a region that ends one base behind the long one, so it is listed right after it, finds it redundant and scoring higher at
    # its first step back (the stopper) and goes
    Lc = rng.integers(0, 4, size=161, dtype=np.uint8)
    Lc[0] = first_e
    re_ = Lc[:160].copy()
    for m in (40, 66, 85, 104, 107, 133, 152):
        re_[m] = _other(Lc[m])
    re_[19:40] = Lc[140:161]
    re_[18] = _other(Lc[18], Lc[139])
    Lc[19:40] = Lc[140:161]
    for m in (19, 26, 33):
        Lc[m] = _other(Lc[m])
    for j in range(66):
        s0[p0 - 1] = _other(X[-1])
        s0[p0:p0 + 161] = Lc
        s0[p0 + 161] = _other(re_[40])
        p0 += 450
    for r in (re_, np.concatenate([X, re_])):
        add("redun", r, chain_read(29))
        add("redun", _rc(chain_read(30)), _rc(r))
    assert p0 < len(s0) - 1000, p0
    # ---- contig 1: pair families
    pp = [2000]

    def pair_family(loci, diverged, mirrored=False, gap=100, kind_="rescue", r1_exact=100, special=(), every=8):
        """loci copies of [read 1's 100 bases][gap][reverse complement of read 2's 100 bases] (mirrored: the pair on the other strand)."""
        a1 = rng.integers(0, 4, size=100, dtype=np.uint8)
        a2 = rng.integers(0, 4, size=100, dtype=np.uint8)
        # read 2's list is sorted by score, then by position on its own strand: the reverse strand's first entries are the genome's last loci
        first = set(range(loci - diverged, loci)) if not mirrored else set(range(diverged))
        spec = set((loci - 1 - k) if not mirrored else k for k in special)
        for j in range(loci):
            p = pp[0]
            c1 = a1.copy()
            if r1_exact < 100 and j not in spec:
                c1[r1_exact] = _other(c1[r1_exact])
                c1[r1_exact + 1:] = rng.integers(0, 4, size=99 - r1_exact, dtype=np.uint8)
            if j in first or j in spec:
                step = every if j in first else 16
                for k in range(step - 1, 100, step):
                    c1[k] = (c1[k] + 1 + (k + j) % 3) % 4
            s1[p:p + 100] = c1
            s1[p + 100 + gap:p + 200 + gap] = a2
            pp[0] = p + max(420, gap + 300)
        # ... and once more with the two reads swapped: the same insertions, made by the second rescue loop
        if mirrored:
            add(kind_, _rc(a2), a1)
            add(kind_, a1, _rc(a2))
        else:
            add(kind_, a1, _rc(a2))
            add(kind_, _rc(a2), a1)

    pair_family(66, 3)
    pair_family(66, 3, mirrored=True)
    pair_family(130, 4)
    pair_family(264, 14)
    pair_family(70, 0, kind_="first", r1_exact=45, special=(1, 5, 9))
    pair_family(66, 0, gap=306, kind_="far")
    pair_family(66, 0, gap=380, kind_="far")
    pair_family(66, 0, gap=340, mirrored=True, kind_="far")
    assert pp[0] < len(s1) - 1000, pp[0]
    # ---- ordinary traffic
    rs = nasty_reads(seed, g, n_barcodes=2, pairs_per_barcode=nasty_pairs // 2)
    for i in range(rs.seqs.shape[0] // 2):
        add("nasty", rs.seqs[2 * i, :rs.lens[2 * i]], rs.seqs[2 * i + 1, :rs.lens[2 * i + 1]])
    order = rng.permutation(len(pairs))
    reads = [r for i in order for r in pairs[i]]
    rk = np.array([kind[i] for i in order for _ in (0, 1)])
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    kinds = {k: np.nonzero(rk == k)[0] for k in ("chain", "cap", "rank", "redun", "rescue", "first", "far", "nasty")}
    flat = np.concatenate(reads)
    assert flat.max() <= 4 and lens.max() <= 255
    return g, flat, lens, kinds

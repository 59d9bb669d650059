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

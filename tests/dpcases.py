"""Seeded cases for the three DP kernel families (banded extension, rescue Smith-Waterman, CIGAR global alignment), the layout that hands them
to the library's self-test entries (reference text in .pac layout, doubled coordinates, both strands and directions), the oracle's answer
for each (ksw_extend2 / ksw_align2 / ksw_global2 of oracle/liboracle.so) and the coverage counts the test modules assert.

Used by tests/test_dp_cases_hostsim.py (the serial forms in the host test double) and tests/test_dp_kernels_gpu.py (the kernels)."""
import numpy as np

EB, ZDROP = 5, 100                       # end bonus (pen_clip5) and z-drop of the path
KSW_XBYTE, KSW_XSUBO, KSW_XSTART = 0x10000, 0x40000, 0x80000
MIN_SEED_LEN = 19
SW_T_CAP, NW_Q_CAP, NW_T_CAP, EXT_T_CAP = 800, 256, 1024, 512
NW_HI = (2, 4, 8, 16, 16, 16)            # widest tiling (columns per lane) of CIGAR kernels 0..4 and of the <1,16> kernel (5)
EXT_BOUNDS = (32, 48, 64, 96, 128, 160)  # arx_dev.h ext_class
NONE_U8 = np.array([0, -1, -1, -1, -1, -1, -1], dtype=np.int32)   # what a task the rescue pre-filter drops returns


def ext_class(qlen):
    return int(np.searchsorted(EXT_BOUNDS, qlen, side="right"))


def revcomp(s):
    s = np.asarray(s, dtype=np.uint8)
    return np.where(s < 4, 3 - s, 4).astype(np.uint8)[::-1].copy()


def rand_seq(rng, n):
    return rng.integers(0, 4, size=int(n), dtype=np.uint8)


def mutate(rng, s, sub=0.04, indel=0.01, max_gap=6):
    out = []
    i = 0
    s = np.asarray(s, dtype=np.uint8)
    while i < len(s):
        r = rng.random()
        if r < indel / 2:                                 # deletion from s
            i += int(rng.integers(1, max_gap + 1))
            continue
        if r < indel:                                     # insertion
            out.extend(rand_seq(rng, rng.integers(1, max_gap + 1)).tolist())
        b = int(s[i])
        if rng.random() < sub:
            b = (b + int(rng.integers(1, 4))) & 3 if b < 4 else int(rng.integers(0, 4))
        out.append(b)
        i += 1
    return np.array(out, dtype=np.uint8)


def no_n(s):
    s = np.asarray(s, dtype=np.uint8).copy()
    s[s > 3] = 0
    return s


class Text:
    """A forward text assembled from placed pieces with random spacers between them; .pac layout (2 bits per base, first base in the top
    bits).  add() returns a handle whose doubled coordinate is resolved by finish(): a target read forward or backward, on either strand."""

    def __init__(self, rng):
        self.rng = rng
        self.parts = []
        self.n = 0
        self.pending = []

    def _put(self, seq):
        gap = int(self.rng.integers(0, 9)) if self.parts else 0
        if gap:
            self.parts.append(rand_seq(self.rng, gap))
            self.n += gap
        s = self.n
        self.parts.append(np.asarray(seq, dtype=np.uint8))
        self.n += len(seq)
        return s

    def add(self, t, strand, tdir):
        """t (bases 0..3) as read from the returned position p: base i at p + i * tdir; strand 1 puts p in [l_pac, 2 l_pac)."""
        t = np.asarray(t, dtype=np.uint8)
        L = len(t)
        if strand == 0:
            s = self._put(t if tdir == 1 else t[::-1])
            pos = (lambda Lp, s=s: s) if tdir == 1 else (lambda Lp, s=s, L=L: s + L - 1)
        else:
            s = self._put(revcomp(t) if tdir == 1 else 3 - t)
            pos = (lambda Lp, s=s, L=L: 2 * Lp - s - L) if tdir == 1 else (lambda Lp, s=s: 2 * Lp - 1 - s)
        self.pending.append(pos)
        return len(self.pending) - 1

    def finish(self):
        self.parts.append(rand_seq(self.rng, 3))          # the last piece may still touch the end of the text
        fwd = np.concatenate(self.parts)
        self.l_pac = len(fwd)
        pad = np.zeros((len(fwd) + 3) // 4 * 4, dtype=np.uint8)
        pad[:len(fwd)] = fwd
        p4 = pad.reshape(-1, 4).astype(np.uint8)
        self.pac = (p4[:, 0] << 6 | p4[:, 1] << 4 | p4[:, 2] << 2 | p4[:, 3]).astype(np.uint8)
        self.fwd = fwd
        self.pos = [f(self.l_pac) for f in self.pending]
        return self

    def base(self, p):   # ref_base of arx_dev.h, for checking the layout itself
        return int(self.fwd[p]) if p < self.l_pac else 3 - int(self.fwd[2 * self.l_pac - 1 - p])


# ---------------------------------------------------------------------------------------------------------------------------------------
# extension: ksw_extend2(q, t, w, 5, 100, h0)
# ---------------------------------------------------------------------------------------------------------------------------------------
QLEN_EDGES = (1, 2, 15, 16, 17, 31, 32, 47, 48, 63, 64, 95, 96, 127, 128, 159, 160, 161, 200, 254, 255)


def _ext_one(rng, kind, qlen=None):
    """one (q, t, w, h0) of a kind"""
    w = int(rng.choice([100, 200]))
    h0 = int(rng.integers(5, 80))
    if qlen is None:
        qlen = int(rng.integers(1, 256))
    q = rand_seq(rng, qlen)
    if kind == "related":
        t = np.concatenate([no_n(mutate(rng, q, 0.05, 0.02)), rand_seq(rng, rng.integers(0, 120))])
    elif kind == "long_t":                                # tlen at and beyond the LDS staging cap of the kernel
        q = rand_seq(rng, int(rng.integers(180, 256)))
        tl = int(rng.choice([511, 512, 513, int(rng.integers(514, 1100))]))
        t = np.concatenate([no_n(mutate(rng, q, 0.01, 0.01, 3)), rand_seq(rng, tl)])[:tl]
        w = int(rng.choice([100, 200, 255]))
    elif kind == "short_t":
        t = rand_seq(rng, int(rng.integers(1, 4)))
        if rng.random() < 0.5:
            t[:] = q[:len(t)] if len(q) >= len(t) else t
    elif kind == "small_w":                               # the band drops columns: gaps longer than w
        w = int(rng.integers(1, 9))
        t = np.concatenate([no_n(mutate(rng, q, 0.03, 0.06, 14)), rand_seq(rng, rng.integers(0, 40))])
    elif kind == "big_w":                                 # w above qlen: clamped
        w = qlen + int(rng.integers(1, 400))
        t = np.concatenate([no_n(mutate(rng, q, 0.05, 0.03, 10)), rand_seq(rng, rng.integers(0, 60))])
    elif kind == "h0":                                    # large h0, short query
        q = rand_seq(rng, int(rng.integers(1, 31)))
        h0 = int(rng.integers(1, 256))
        t = no_n(mutate(rng, q, 0.1, 0.05)) if rng.random() < 0.6 else rand_seq(rng, rng.integers(1, 60))
        if len(t) == 0:
            t = rand_seq(rng, 1)
    elif kind == "zdrop_del":                             # strong match, then the target goes on with extra sequence: deletion side
        a = rand_seq(rng, int(rng.integers(100, 200)))
        b = rand_seq(rng, int(rng.integers(10, 50)))
        q = np.concatenate([a, b])[:255]
        t = np.concatenate([a, rand_seq(rng, rng.integers(20, 160)), b, rand_seq(rng, rng.integers(0, 30))])
        w = int(rng.choice([5, 10, 20, 40, 100]))
    elif kind == "zdrop_ins":                             # ... the query holds extra sequence: insertion side
        a = rand_seq(rng, int(rng.integers(100, 180)))
        x = rand_seq(rng, int(rng.integers(20, 70)))
        b = rand_seq(rng, int(rng.integers(5, 30)))
        q = np.concatenate([a, x, b])[:255]
        t = np.concatenate([a, b, rand_seq(rng, rng.integers(50, 200))])
        w = int(rng.choice([5, 10, 20, 40, 100]))
    elif kind == "early":                                 # a strong early match, then noise: the dead-row exit
        m = int(rng.integers(15, 70))
        q = np.concatenate([rand_seq(rng, m), rand_seq(rng, rng.integers(20, 180))])[:255]
        t = np.concatenate([q[:m], rand_seq(rng, rng.integers(100, 500))])
        h0 = int(rng.integers(1, 40))
    elif kind == "lowc":                                  # low-complexity runs: tied row maxima, tied gscore rows
        unit = rand_seq(rng, int(rng.integers(1, 4)))
        q = np.tile(unit, 256)[:qlen].copy()
        t = np.tile(unit, 600)[:int(rng.integers(max(1, qlen - 20), qlen + 80))].copy()
        for _ in range(int(rng.integers(0, 3))):
            t[int(rng.integers(0, len(t)))] = int(rng.integers(0, 4))
    else:
        raise ValueError(kind)
    if kind not in ("h0",) and rng.random() < 0.08:       # N in the query
        q = q.copy()
        q[rng.integers(0, len(q), size=int(rng.integers(1, 4)))] = 4
    return q, np.ascontiguousarray(t, dtype=np.uint8), w, h0


def ext_cases(seed, n_random=1500, golden=None):
    """a list of dicts (q, t, w, h0, qdir, tdir, strand, kind).  golden: the npz of the compiled reference's vectors; its cases with the
    path's parameters (end bonus 5, z-drop 100) come first."""
    rng = np.random.default_rng(seed)
    cases = []

    def push(q, t, w, h0, kind):
        cases.append(dict(q=q, t=t, w=int(w), h0=int(h0), qdir=int(rng.choice([1, -1])), tdir=int(rng.choice([1, -1])), strand=int(rng.integers(0, 2)), kind=kind))

    if golden is not None:
        for i, q, t in golden_sw(golden):
            w, eb, zd, h0 = (int(x) for x in golden["sw_ext_par"][i])
            if eb == EB and zd == ZDROP and 1 <= h0 <= 255 and 1 <= len(q) <= 255 and len(t) >= 1 and w >= 1 and (t < 4).all():   # (the text holds no N)
                push(q, t, w, h0, "golden")
    for ql in QLEN_EDGES:                                 # every class boundary, a few times over
        for _ in range(6):
            push(*_ext_one(rng, "related", ql), "edge")
    kinds = ["related", "long_t", "short_t", "small_w", "big_w", "h0", "zdrop_del", "zdrop_ins", "early", "lowc"]
    for k in range(n_random):
        push(*_ext_one(rng, kinds[k % len(kinds)]), kinds[k % len(kinds)])
    for k in range(40):                                   # four tasks of very different lengths next to each other, in one class
        c = k % 7
        lo, hi = ([1] + list(EXT_BOUNDS))[c], (list(EXT_BOUNDS) + [256])[c] - 1
        for tl in (1, 37, 300, 700):
            q = rand_seq(rng, int(rng.choice([lo, hi])))
            t = np.concatenate([no_n(mutate(rng, q)), rand_seq(rng, tl)])[:tl]
            push(q, t, 100, int(rng.integers(1, 60)), "wave4")
    # a window that ends at, or up to three bases beyond, the seed (fetch_clamp at a contig's edge; tlen == 0: rmax0 == seed.rbeg): at every class
    # boundary, with the first target bases matching and not, both bands
    for ql in QLEN_EDGES:
        for tl in (0, 1, 2, 3):
            for match in (0, 1):
                q = rand_seq(rng, ql)
                t = rand_seq(rng, tl)
                if match:
                    t[:min(tl, ql)] = q[:min(tl, ql)]
                push(q, t, (100, 200)[(tl + match) & 1], int(rng.integers(1, 256)), "edge_t")
    return cases


def ext_layout(cases, seed):
    """-> (pac, l_pac, bases, tasks n x 8) for arx_selftest_extend / arx_test_ext2_task"""
    rng = np.random.default_rng(seed + 7)
    text = Text(rng)
    handles = [text.add(c["t"], c["strand"], c["tdir"]) for c in cases]
    text.finish()
    bases, tasks, at = [], np.zeros((len(cases), 8), dtype=np.int64), 0
    for i, c in enumerate(cases):
        q = c["q"]
        bases.append(q if c["qdir"] == 1 else q[::-1])
        qoff = at if c["qdir"] == 1 else at + len(q) - 1
        at += len(q)
        tasks[i] = (text.pos[handles[i]], qoff, len(q), len(c["t"]), c["qdir"], c["tdir"], c["w"], c["h0"])
    return text, np.concatenate(bases).astype(np.uint8), tasks


def ext_oracle(o, cases):
    return np.array([o.ksw_extend2(c["q"], c["t"], c["w"], EB, ZDROP, c["h0"]) for c in cases], dtype=np.int32).reshape(-1, 6)


def ext_coverage(cases, exp):
    """what the extension cases reach, from inputs and oracle outputs (score, qle, tle, gtle, gscore, max_off)"""
    ql = np.array([len(c["q"]) for c in cases])
    tl = np.array([len(c["t"]) for c in cases])
    w = np.array([c["w"] for c in cases])
    h0 = np.array([c["h0"] for c in cases])
    cls = np.array([ext_class(x) for x in ql])
    return dict(
        per_class=[int((cls == c).sum()) for c in range(7)],
        qlen_edges=sorted(set(int(x) for x in ql) & set(QLEN_EDGES)),
        qlen_255=int((ql == 255).sum()),
        tlen_0=int((tl == 0).sum()), tlen_0_classes=sorted(set(int(x) for x in cls[tl == 0])), tlen_2_3=int(((tl == 2) | (tl == 3)).sum()),
        tlen_1=int((tl == 1).sum()), tlen_511_513=sorted(set(int(x) for x in tl) & {511, 512, 513}), tlen_over_512=int((tl > EXT_T_CAP).sum()),
        both_dirs_strands=len({(c["qdir"], c["tdir"], c["strand"]) for c in cases}),
        w_100=int((w == 100).sum()), w_200=int((w == 200).sum()), w_small=int((w < 10).sum()), w_over_qlen=int((w > ql).sum()),
        h0_over_200_short_q=int(((h0 > 200) & (ql <= 30)).sum()),
        n_in_query=int(sum(int((c["q"] > 3).any()) for c in cases)),
        gscore_neg=int((exp[:, 4] == -1).sum()), gtle_below_tlen=int((exp[:, 3] < tl).sum()),
        max_off_half_w=int((exp[:, 5] >= np.minimum(w, ql) / 2).sum()),
        score_h0_only=int(((exp[:, 0] == h0) & (exp[:, 2] == 0)).sum()),
        stopped_early=int(((exp[:, 2] < tl - 40) & (exp[:, 0] > h0 + 60)).sum()),     # a long match, then rows left unread: z-drop or the band
    )


# ---------------------------------------------------------------------------------------------------------------------------------------
# rescue SW: ksw_align2(revcomp(mate), window, XSUBO | XSTART | (XBYTE iff l_ms < 250) | 19)
# ---------------------------------------------------------------------------------------------------------------------------------------
MATE_EDGES = (1, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 96, 97, 128, 129, 159, 160, 161, 175, 176, 177, 191, 192, 193, 223, 224,
              225, 240, 249, 250, 251, 254, 255)


def sw_xtra(l_ms):
    return KSW_XSUBO | KSW_XSTART | (KSW_XBYTE if l_ms < 250 else 0) | MIN_SEED_LEN


def _sw_one(rng, kind, l_ms):
    mate = rand_seq(rng, l_ms)
    q = revcomp(mate)                                    # what the DP aligns
    tl = int(rng.integers(max(1, l_ms // 2), SW_T_CAP + 1))
    if kind == "planted":
        t = rand_seq(rng, tl)
        piece = no_n(mutate(rng, q, 0.03, 0.02))[:tl]
        p = int(rng.integers(0, tl - len(piece) + 1))
        t[p:p + len(piece)] = piece
    elif kind == "threshold":                            # a run of 17..21 matches: scores of 18, 19, 20 around the second pass's threshold
        tl = int(rng.integers(40, 300))
        t = rand_seq(rng, tl)
        k = int(rng.integers(17, 22))
        if l_ms >= k:
            a = int(rng.integers(0, l_ms - k + 1))
            p = int(rng.integers(0, tl - k + 1))
            t[p:p + k] = q[a:a + k]
    elif kind == "twice":                                # the same hit twice, far apart: score2 == score
        piece = no_n(q[:min(l_ms, 60)])
        gap = int(rng.integers(len(piece) + 10, 300))
        t = np.concatenate([rand_seq(rng, rng.integers(0, 50)), piece, rand_seq(rng, gap), piece, rand_seq(rng, rng.integers(0, 50))])[:SW_T_CAP]
    elif kind == "short_t":                              # odd windows shorter than the mate
        tl = max(1, int(rng.integers(1, max(2, l_ms))) | 1)
        t = no_n(q[:tl]).copy() if rng.random() < 0.5 else rand_seq(rng, tl)
    elif kind == "long_t":
        tl = int(rng.choice([783, 784, 785, 799, 800]))
        t = rand_seq(rng, tl)
        piece = no_n(mutate(rng, q, 0.02, 0.01))[:tl]
        p = int(rng.choice([0, tl - len(piece), int(rng.integers(0, tl - len(piece) + 1))]))
        t[p:p + len(piece)] = piece
    elif kind == "random":
        t = rand_seq(rng, tl)
    elif kind == "lowc":
        unit = rand_seq(rng, int(rng.integers(1, 4)))
        mate = revcomp(np.tile(unit, 256)[:l_ms])
        t = np.tile(unit, 900)[:tl].copy()
        for _ in range(int(rng.integers(0, 4))):
            t[int(rng.integers(0, tl))] ^= 1
    else:
        raise ValueError(kind)
    if rng.random() < 0.08:                              # N in the mate
        mate = mate.copy()
        mate[rng.integers(0, l_ms, size=int(rng.integers(1, 3)))] = 4
    return mate, np.ascontiguousarray(t, dtype=np.uint8)


def sw_cases(seed, n_random=1200, golden=None):
    rng = np.random.default_rng(seed)
    cases = []

    def push(mate, t, kind):
        cases.append(dict(mate=np.asarray(mate, dtype=np.uint8), t=t, strand=int(rng.integers(0, 2)), kind=kind))

    if golden is not None:                               # the reference's own ksw_align2 vectors (query = the reverse complement of a mate)
        for i, q, t in golden_sw(golden):
            if 1 <= len(q) <= 255 and 1 <= len(t) <= SW_T_CAP and (t < 4).all():
                push(revcomp(q), np.ascontiguousarray(t, dtype=np.uint8), "golden")
    kinds = ["planted", "threshold", "twice", "short_t", "long_t", "random", "lowc"]
    for l_ms in MATE_EDGES:
        for k in range(len(kinds)):
            push(*_sw_one(rng, kinds[k], l_ms), kinds[k])
    for k in range(n_random):
        l_ms = int(rng.integers(1, 256)) if k % 3 else int(rng.choice(MATE_EDGES))
        push(*_sw_one(rng, kinds[k % len(kinds)], l_ms), kinds[k % len(kinds)])
    return cases


def sw_layout(cases, seed):
    """-> (text, mates, mate_off, mate_len, windows n x 2) for arx_selftest_rescue_sw: window i reads forward on its strand"""
    rng = np.random.default_rng(seed + 11)
    text = Text(rng)
    handles = [text.add(c["t"], c["strand"], 1) for c in cases]
    text.finish()
    ml = np.array([len(c["mate"]) for c in cases], dtype=np.int32)
    mo = np.concatenate([[0], np.cumsum(ml)[:-1]]).astype(np.int32)
    win = np.array([(text.pos[h], text.pos[h] + len(c["t"])) for h, c in zip(handles, cases)], dtype=np.int64).reshape(-1, 2)
    return text, np.concatenate([c["mate"] for c in cases]).astype(np.uint8), mo, ml, win


def sw_oracle(o, cases):
    return np.array([o.ksw_align2(revcomp(c["mate"]), c["t"], sw_xtra(len(c["mate"]))) for c in cases], dtype=np.int32).reshape(-1, 7)


def sw_coverage(cases, exp):
    ml = np.array([len(c["mate"]) for c in cases])
    tl = np.array([len(c["t"]) for c in cases])
    return dict(
        mates_16k_edges=sorted(set(int(x) for x in ml) & {15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 191, 192, 193, 223, 224, 225}),
        mates_160_161=sorted(set(int(x) for x in ml) & {160, 161}), mates_249_255=sorted(set(int(x) for x in ml) & {249, 250, 255}),
        i16=int((ml >= 250).sum()),
        odd_tlen=int((tl % 2 == 1).sum()), tlen_below_qlen=int((tl < ml).sum()), tlen_784_800=sorted(set(int(x) for x in tl) & {784, 800}),
        score_18=int((exp[:, 0] == 18).sum()), score_19=int((exp[:, 0] == 19).sum()), score_20=int((exp[:, 0] == 20).sum()),
        score2_eq_score=int(((exp[:, 3] == exp[:, 0]) & (exp[:, 0] > 0)).sum()),
        tb_qb_set=int((exp[:, 5] >= 0).sum()), reverse_strand=int(sum(c["strand"] for c in cases)),
        n_in_mate=int(sum(int((c["mate"] > 3).any()) for c in cases)),
    )


# ---------------------------------------------------------------------------------------------------------------------------------------
# CIGAR: bwa_gen_cigar2 -> ksw_global2(q, t, w) with w from its band formula; NM by bwa.c's rule
# ---------------------------------------------------------------------------------------------------------------------------------------
def gen_cigar_band(l_query, rlen, w_):
    """bwa_gen_cigar2's band (bwa.c:150-156) with a = 1, o = 6, e = 1 -> (w, n_col)"""
    max_gap = max(((l_query + 1) >> 1) - 5, 1)
    w = min((max_gap + abs(rlen - l_query) + 1) >> 1, w_)
    w = max(w, abs(rlen - l_query) + 3)
    return w, min(l_query, 2 * w + 1)


def nw_tiling(n_col):
    return 1 if n_col <= 16 else 2 if n_col <= 32 else 4 if n_col <= 64 else 8 if n_col <= 128 else 16


def sc_mat(t, q):
    return -1 if (t > 3 or q > 3) else (1 if t == q else -4)


def nm_of(q, t, cig):
    """bwa_gen_cigar2's NM (bwa.c:169-199): mismatches in M runs plus inserted and deleted bases; a leading or trailing D is not counted"""
    x = y = nm = 0
    n = len(cig)
    for k, c in enumerate(cig):
        op, ln = int(c) & 0xf, int(c) >> 4
        if op == 0:
            nm += int((q[x:x + ln] != t[y:y + ln]).sum())
            x += ln
            y += ln
        elif op == 2:
            if 0 < k < n - 1:
                nm += ln
            y += ln
        elif op == 1:
            x += ln
            nm += ln
    return nm


def _nw_one(rng, kind):
    ql = int(rng.integers(1, NW_Q_CAP + 1))
    q = rand_seq(rng, ql)
    w_ = int(rng.choice([0, 1, 3, 8, 20, 50, 100, 200, 400]))
    if kind == "related":
        t = no_n(mutate(rng, q, 0.04, 0.03, 8))
    elif kind == "wide":                                 # long indels: wide bands, the wide tilings
        t = no_n(mutate(rng, q, 0.02, 0.02, 40))
        w_ = int(rng.choice([50, 100, 200, 400]))
    elif kind == "ends":                                 # indels at both ends
        t = no_n(q.copy())
        lt, rt = rand_seq(rng, rng.integers(0, 15)), rand_seq(rng, rng.integers(0, 15))
        if rng.random() < 0.5:
            t = np.concatenate([lt, t, rt])
        else:
            a, b = int(rng.integers(0, min(15, ql) + 1)), int(rng.integers(0, min(15, ql) + 1))
            t = t[a:len(t) - b] if len(t) - a - b >= 1 else t
        w_ = int(rng.choice([5, 20, 100]))
    elif kind == "gapfree":                              # the shortcut: l_query == rlen, w_ == 0
        t = no_n(q.copy())
        m = rng.random(ql) < 0.05
        t[m] = (t[m] + 1) & 3
        w_ = 0
    elif kind == "equal_len":                            # equal lengths, but a band: the DP
        t = no_n(q.copy())
        m = rng.random(ql) < 0.05
        t[m] = (t[m] + 1) & 3
        w_ = int(rng.integers(1, 30))
    elif kind == "long_t":
        t = np.concatenate([rand_seq(rng, rng.integers(0, 400)), no_n(mutate(rng, q, 0.03, 0.03, 10)), rand_seq(rng, rng.integers(0, 400))])[:NW_T_CAP]
        w_ = int(rng.choice([100, 200, 400]))
    elif kind == "random":
        t = rand_seq(rng, rng.integers(1, 2 * ql + 10))
    else:
        raise ValueError(kind)
    if len(t) == 0:
        t = rand_seq(rng, 1)
    if rng.random() < 0.08:                              # N in the query
        q = q.copy()
        q[rng.integers(0, ql, size=int(rng.integers(1, 4)))] = 4
    return q, np.ascontiguousarray(t[:NW_T_CAP], dtype=np.uint8), w_


def nw_cases(seed, n_random=900, golden=None):
    rng = np.random.default_rng(seed)
    cases = []
    if golden is not None:                               # the reference's ksw_global2 vectors: a w_ for which the band formula gives their w
        off = golden["sw_glo_off"]
        for i, q, t in golden_sw(golden):
            w_gold = int(golden["sw_glo_par"][i][0])
            if not (1 <= len(q) <= NW_Q_CAP and 1 <= len(t) <= NW_T_CAP and (t < 4).all()):
                continue
            for w_ in range(1, 401):
                if gen_cigar_band(len(q), len(t), w_)[0] == w_gold:
                    cases.append(dict(q=np.asarray(q, dtype=np.uint8), t=np.asarray(t, dtype=np.uint8), w_=w_, cap=1024, kind="golden",
                                      gold=(int(golden["sw_glo_par"][i][1]), golden["sw_glo_cig"][off[i]:off[i + 1]])))
                    break
    kinds = ["related", "wide", "ends", "gapfree", "equal_len", "long_t", "random"]
    for k in range(n_random):
        q, t, w_ = _nw_one(rng, kinds[k % len(kinds)])
        cases.append(dict(q=q, t=t, w_=w_, cap=1024, kind=kinds[k % len(kinds)]))
    for k in range(60):                                  # a cap smaller than the CIGAR
        q, t, w_ = _nw_one(rng, "related")
        cases.append(dict(q=q, t=t, w_=max(w_, 1), cap=int(rng.integers(1, 4)), kind="cap"))
    return cases


def nw_oracle(o, c):
    """-> (score, cigar words, NM) of bwa_gen_cigar2 for one case (NM -1 when the CIGAR does not fit cap)"""
    q, t = c["q"], c["t"]
    if len(q) == len(t) and c["w_"] == 0:
        sc = sum(sc_mat(int(a), int(b)) for a, b in zip(t, q))
        cig = np.array([len(q) << 4], dtype=np.uint32)
    else:
        w, _ = gen_cigar_band(len(q), len(t), c["w_"])
        sc, cig = o.ksw_global2(q, t, w, cap=4096)
    return int(sc), cig, (nm_of(q, t, cig) if len(cig) <= c["cap"] else -1)


def nw_coverage(cases, exp):
    cols = [gen_cigar_band(len(c["q"]), len(c["t"]), c["w_"])[1] for c in cases]
    shortcut = [len(c["q"]) == len(c["t"]) and c["w_"] == 0 for c in cases]
    til = [0 if s else nw_tiling(n) for n, s in zip(cols, shortcut)]
    lead = sum(1 for sc, cg, nm in exp if len(cg) > 1 and (int(cg[0]) & 0xf) in (1, 2))
    trail = sum(1 for sc, cg, nm in exp if len(cg) > 1 and (int(cg[-1]) & 0xf) in (1, 2))
    return dict(
        per_tiling={k: til.count(k) for k in (1, 2, 4, 8, 16)},
        punts_per_kernel=[sum(1 for n, s in zip(cols, shortcut) if not s and n > 16 * NW_HI[k]) for k in range(6)],
        gapfree_shortcut=int(sum(shortcut)), lead_indel=lead, trail_indel=trail,
        n_in_query=int(sum(int((c["q"] > 3).any()) for c in cases)),
        nm_minus1=int(sum(1 for e in exp if e[2] == -1)),
        qlen_256=int(sum(1 for c in cases if len(c["q"]) == NW_Q_CAP)), tlen_over_512=int(sum(1 for c in cases if len(c["t"]) > 512)),
    )


def golden_sw(z):
    qo = np.concatenate([[0], np.cumsum(z["sw_qlen"])])
    to = np.concatenate([[0], np.cumsum(z["sw_tlen"])])
    for i in range(len(z["sw_qlen"])):
        yield i, np.ascontiguousarray(z["sw_q"][qo[i]:qo[i + 1]]), np.ascontiguousarray(z["sw_t"][to[i]:to[i + 1]])

"""Chaining by 16-lane groups (k_chain_g16, dev_chain_group.h) against the thread-per-read path and the oracle (-m gpu).

With ARX_CHAIN_GROUP=1 the group kernel chains every read with 1-63 seed occurrences; by default KChain / KChainMid chain them, one
thread each.
  * whole batch: debug_chains() and fetch() of both paths, byte for byte, and the "chain" scope's launch count showing that the group
    launches ran (KChain leaves the group classes' reads alone, so only k_chain_g16 can have chained them);
  * reads at the class edges (1, 2, 3, 9, 10, 16, 17, 63, 64 occurrences) against the oracle's mem_chain + mem_chain_flt, also with
    ARX_CHAIN_HEAVY_MIN raised so that the group kernel's largest class takes reads the heavy kernel would otherwise have;
  * the coverage the equality rests on, asserted and printed: reads with three or more chains of equal weight (klib's partition decides
    their order), reads with ten or more chains (the B-tree splits), reads whose chains share a position (duplicate keys).
"""
import os
import tempfile

import numpy as np
import pytest

import parity
from arachne_amd import api, synth

pytestmark = pytest.mark.gpu

EDGES = (1, 2, 3, 9, 10, 16, 17, 63, 64)


@pytest.fixture(scope="module")
def env(built):
    import oradrv
    # a 200-copy 3 kb family beside 60 copies of 2 kb at 1 % divergence and short repeats: reads with 1 to several hundred occurrences
    g = synth.make_genome(91, [3_000_000, 40000], repeat_families=[(200, 3000, 0.01), (60, 2000, 0.0), (400, 300, 0.12)], n_runs=1)
    rs = synth.make_reads(92, g, 6, 400, molecule_len=20000, molecules_per_barcode=6)
    for i in range(0, len(rs.lens), 50):   # the read's first 40 bases again at its end: two seeds at one position, 110 query bases apart
        s = np.array(rs.seqs[i], dtype=np.uint8)
        s[110:150] = s[0:40]
        rs.seqs[i] = s
    d = tempfile.mkdtemp(prefix="arx_chain_g16_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    api.index_build(fa, fa)
    ref = api.Reference(fa)
    o = oradrv.Oracle(fa)
    yield ref, o, rs
    ref.close()
    o.close()


def _valid(occ_off, n_chain, ch, sd):
    """The chains each read kept and their seeds (the rest of the per-read slices is scratch)."""
    starts = np.repeat(occ_off[:-1].astype(np.int64), n_chain)
    within = np.arange(len(starts)) - np.repeat(np.cumsum(n_chain) - n_chain, n_chain)
    c = ch[starts + within]
    s_start = np.repeat(c["seed_off"].astype(np.int64), c["n"])
    s_within = np.arange(len(s_start)) - np.repeat(np.cumsum(c["n"]) - c["n"], c["n"])
    return c, sd[s_start + s_within]


def _run(ref, rs, monkeypatch, group, heavy_min=None):
    if group:
        monkeypatch.setenv("ARX_CHAIN_GROUP", "1")
    else:
        monkeypatch.delenv("ARX_CHAIN_GROUP", raising=False)
    if heavy_min is None:
        monkeypatch.delenv("ARX_CHAIN_HEAVY_MIN", raising=False)
    else:
        monkeypatch.setenv("ARX_CHAIN_HEAVY_MIN", str(heavy_min))
    ref.kernel_times_reset(True)
    try:
        b = ref.batch(rs.seqs, rs.lens).run()
        occ_off, n_chain, ch, sd = b.debug_chains()
        occ_off = occ_off.copy()
        out = b.fetch()
        chain = ref.kernel_times()["chain"]
    finally:
        ref.kernel_times_reset(False)
    # the "chain" scope: KChain's launch (one item per read), then run_chain_group's (one per read) or KChainMid's (its list's capacity)
    n = len(rs.lens)
    if group:
        assert chain["calls"] == 2 and chain["items"] == 2 * n, chain
    else:
        assert chain["items"] != 2 * n, chain
    return b, occ_off, n_chain.copy(), ch.copy(), sd.copy(), out


def _coverage(occ_off, n_chain, ch):
    n_occ = np.diff(occ_off)
    ties = many = dup = 0
    for r in np.nonzero((n_occ >= 1) & (n_occ <= 63) & (n_chain > 0))[0]:
        c = ch[occ_off[r]:occ_off[r] + n_chain[r]]
        if np.unique(c["w"], return_counts=True)[1].max() >= 3:
            ties += 1
        if n_chain[r] >= 10:
            many += 1
        if len(np.unique(c["pos"])) < len(c):
            dup += 1
    return ties, many, dup


def test_group_path_equals_thread_per_read_path(env, monkeypatch):
    ref, o, rs = env
    b0, off0, n0, ch0, sd0, out0 = _run(ref, rs, monkeypatch, group=False)
    b0.free()
    b1, off1, n1, ch1, sd1, out1 = _run(ref, rs, monkeypatch, group=True)
    b1.free()
    assert np.array_equal(off0, off1)
    assert np.array_equal(n0, n1)
    c0, s0 = _valid(off0, n0, ch0, sd0)
    c1, s1 = _valid(off1, n1, ch1, sd1)
    assert c0.tobytes() == c1.tobytes()
    assert s0.tobytes() == s1.tobytes()
    assert out0["counts"] == out1["counts"]
    for k in ("reg_off", "regs", "alns", "cigars"):
        assert out0[k].tobytes() == out1[k].tobytes(), k
    n_occ = np.diff(off1)
    small, mid = int(((n_occ >= 1) & (n_occ <= 16)).sum()), int(((n_occ >= 17) & (n_occ <= 63)).sum())
    ties, many, dup = _coverage(off1, n1, ch1)
    print(f"\ngroup path: {small} reads of 1-16 occurrences, {mid} of 17-63; chains kept {int(n1.sum())}; reads with >= 3 chains of equal "
          f"weight {ties}, with >= 10 chains {many}, with chains sharing a position {dup}")
    assert small > 1000 and mid > 50
    assert ties > 0 and many > 0 and dup > 0


@pytest.mark.parametrize("heavy_min", [None, 128])
def test_class_edges_match_oracle(env, monkeypatch, heavy_min):
    ref, o, rs = env
    b, occ_off, n_chain, ch, sd, _ = _run(ref, rs, monkeypatch, group=True, heavy_min=heavy_min)
    n_occ = np.diff(occ_off)
    picked = []
    for e in EDGES + ((100, 127) if heavy_min else ()):
        at = np.nonzero(n_occ == e)[0]
        if len(at) == 0:   # the nearest count on the same side of the class edge
            lo, hi = (1, 16) if e <= 16 else (17, 63) if e <= 63 else (64, 127)
            cand = np.nonzero((n_occ >= lo) & (n_occ <= hi))[0]
            assert len(cand), e
            at = cand[np.argsort(np.abs(n_occ[cand] - e), kind="stable")[:1]]
        picked.extend(at[:4].tolist())
    print(f"\nclass edges (heavy_min {heavy_min}): occurrence counts checked {sorted(set(int(n_occ[r]) for r in picked))}")
    parity.check_chains(b, o, rs.seqs, rs.lens, reads=picked)
    b.free()

"""The sweep skip and the rank sort of the placement kernel on the GPU.

tests/rfasweeps.py's batch (tests/test_rfa_sweeps_hostsim.py holds its shapes to the restatement) through libarachne_amd.so's arx_selftest_rfa with
ARX_RFA_SKIP_SWEEPS on and off, two calls each in one process: everything equals the restatement, the forms are byte-identical, and the sweeps
a barcode ran are the ones the rule allows.

sort_kv (hip_block.h) around the size up to which it sorts by counting ranks -- one entry per lane, so at most the class's lanes L -- through
arx_selftest_block, against numpy.lexsort on (uint32(value), key): with the class's default threshold, with the bitonic network alone
(ARX_BLOCK_RANK_SORT=0) and with the rank sort up to L whatever the default is."""
import time

import numpy as np
import pytest

import rfacases
import rfasweeps
from arachne_amd import api

pytestmark = pytest.mark.gpu
PAD_K, RANK_SWITCH = ~np.uint64(0), "ARX_BLOCK_RANK_SORT"


@pytest.fixture(scope="module")
def case(built):
    c = rfasweeps.build()
    c["ora"] = rfacases.oracle(c)
    c["census"] = rfasweeps.census(c["ora"], c["bc_pair_off"])
    return c


def test_switch_on_and_off(case, monkeypatch):
    res = []
    for sw in (1, 0, 1, 0):
        monkeypatch.setenv(rfasweeps.SWITCH, str(sw))
        t0 = time.time()
        dev = rfacases.run_device(case, api.LIB_PATH)
        print(f"\n[rfa sweeps gpu] {rfasweeps.SWITCH}={sw}: {time.time() - t0:.2f} s, sweeps per barcode {dev['barcodes']['pad'].tolist()}")
        rfacases.check_device(case, dev, np.zeros(len(case["barcodes"]), dtype=np.uint8))
        res.append(dev)
    for d in res[1:]:
        rfasweeps.same_results(res[0], d)
    rfasweeps.check_sweep_counts(case, res[0], res[1])
    rfasweeps.check_sweep_counts(case, res[2], res[3])
    assert (res[0]["barcodes"]["pad"] == res[2]["barcodes"]["pad"]).all() and (res[1]["barcodes"]["pad"] == res[3]["barcodes"]["pad"]).all()


def _key_sets(P, rng):
    idx = np.arange(P, dtype=np.int64)
    rnd = rng.integers(0, 1 << 63, size=P, dtype=np.uint64)
    two = np.where(rng.random(P) < 0.5, np.uint64(7) << np.uint64(36), np.uint64(3) << np.uint64(36)).astype(np.uint64)
    asc = np.sort(rnd)
    n_real = max(1, (3 * P) // 5)
    tail = np.full(P, PAD_K, dtype=np.uint64)
    tail[:n_real] = (rng.integers(0, 3, size=n_real).astype(np.uint64) << np.uint64(36)) | rng.integers(0, 1 << 20, size=n_real).astype(np.uint64)
    return [("all keys equal", np.full(P, 0x0123456789ABCDEF, dtype=np.uint64), rng.permutation(P)),
            ("all keys and values equal", np.full(P, 5, dtype=np.uint64), np.full(P, 3)),
            ("all padding", np.full(P, PAD_K, dtype=np.uint64), np.full(P, -1)),
            ("sorted", asc, idx),
            ("reversed", asc[::-1].copy(), idx[::-1].copy()),
            ("two keys", two, rng.permutation(P)),
            ("two keys, values repeat and -1", two, rng.integers(-1, 3, size=P)),
            ("random", rnd, rng.permutation(P)),
            ("padded tail", tail, np.where(idx < n_real, idx, -1))]


@pytest.mark.parametrize("klass", [0, 1])
def test_sort_kv_at_the_rank_boundary(built, klass, monkeypatch):
    L, S = api.block_class(klass)
    sizes = sorted({1, 2, L // 16, L // 8, L // 4, L // 2, L, 2 * L})      # class 0: 1, 2, 64, 128, 256, 512, 1024, 2048
    assert 2 * L <= S or klass == 0                                        # the small class's sort stays in LDS (pipeline_rfa.h: the class rule)
    rng = np.random.default_rng(20251021 + klass)
    cases, names = [], []
    for P in sizes:
        for what, k, v in _key_sets(P, rng):
            names.append(f"class {klass} P={P} {what}")
            cases.append(("sort_kv", k, np.asarray(v, dtype=np.int64).astype(np.int32)))
    want = []
    for _, k, v in cases:
        o = np.lexsort((v.view(np.uint32), k))
        want.append((k[o], v[o]))
    for setting in (None, "0", str(L)):
        if setting is None:
            monkeypatch.delenv(RANK_SWITCH, raising=False)
        else:
            monkeypatch.setenv(RANK_SWITCH, setting)
        t0 = time.time()
        got = api.selftest_block(klass, cases)
        print(f"\n[sort_kv] class {klass} ({L} lanes), {RANK_SWITCH}={setting}: {len(cases)} cases in {time.time() - t0:.2f} s")
        for nm, (gk, gv), (wk, wv) in zip(names, got, want):
            assert (gk == wk).all() and (gv == wv).all(), (nm, setting)

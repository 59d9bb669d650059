"""The workgroup primitives the placement kernel is written in (arachne_amd/csrc/hip_block.h: exclusive_scan, sort_kv, argmax) against plain
references, through arx_selftest_block: one case per workgroup, started by k_block_items like rfa_barcode itself, so the LDS layout and the launch
bounds are the product's.  The host test double replaces these three with sequential loops (tests/hostsim/sim.cpp: SimBlock), so the chunked scan
with its one-wave fix-up, the bitonic sort's two storage paths, the cross-wave arg-max and the 256-lane class exist on the GPU only.

Sizes are relative to the class's lanes L and sort entries S (asked of the library; by default class 0: 1024 / 4096, class 1: 256 / 1024).  All cases of a class go up in one
call; the three tests of a class look at its results.  References: numpy cumsum in int64, sorted() on (key, uint32(value)), a Python loop."""
import time

import numpy as np
import pytest

from arachne_amd import api

pytestmark = pytest.mark.gpu
NONE_IDX = 0x7FFFFFFF
BIG = 1 << 50   # a planted maximum; the background keys stay below 2^40


def _scan_cases(L, rng):
    out = []
    for n in (0, 1, 63, 64, 65, L - 1, L, L + 1, 2 * L - 1, 2 * L + 1, 5 * L + 3):
        out.append((f"scan flags n={n}", "scan", None, rng.integers(0, 2, size=n)))
        v = rng.integers(0, (1 << 20) + 1, size=n)
        if n:
            v[rng.integers(0, n)] = 1 << 20
        while int(v.sum()) >= 1 << 31:   # the scan is int32: thin the values out until the total fits, the large ones stay large
            v[rng.random(n) < 0.5] = 0
        out.append((f"scan values<=2^20 n={n}", "scan", None, v))
    return out


def _sort_cases(L, S, klass, rng):
    # the product never gives the small class more than S / 2 candidates (pipeline_rfa.h: the class rule), so its sort stays in LDS: P stops at S there
    sizes = (1, 2, 64, S // 2, S, 2 * S, 4 * S) if klass == 0 else (1, 2, 64, S // 2, S)
    out = []
    for P in sizes:
        idx = np.arange(P, dtype=np.int64)
        rnd = rng.integers(0, 1 << 63, size=P, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=P, dtype=np.uint64)
        out.append((f"sort random P={P}", "sort_kv", rnd, rng.permutation(P)))
        out.append((f"sort equal keys P={P}", "sort_kv", np.full(P, 0x0123456789ABCDEF, dtype=np.uint64), rng.permutation(P)))
        dup_v = rng.integers(-1, 6, size=P)      # -1 is 0xffffffff as the sort compares it: last among equal keys
        dup_v[rng.integers(0, P)] = -1
        out.append((f"sort duplicates with -1 P={P}", "sort_kv", rng.integers(0, 4, size=P).astype(np.uint64) << np.uint64(36), dup_v))
        n_real = max(1, (3 * P) // 5)             # rfa_barcode's padding: ~0 keys, value -1 behind the candidates (unfiltered ones keep their index)
        k = np.full(P, ~np.uint64(0), dtype=np.uint64)
        k[:n_real] = (rng.integers(0, 3, size=n_real).astype(np.uint64) << np.uint64(36)) | rng.integers(0, 1 << 20, size=n_real).astype(np.uint64)
        k[:n_real][rng.random(n_real) < 0.1] = ~np.uint64(0)
        v = np.where(idx < n_real, idx, -1)
        out.append((f"sort padded tail P={P}", "sort_kv", k, v))
        asc = np.sort(rnd)
        out.append((f"sort sorted P={P}", "sort_kv", asc, idx))
        out.append((f"sort reversed P={P}", "sort_kv", asc[::-1].copy(), idx[::-1].copy()))
    return out


def _argmax_cases(L, rng):
    out = []

    def bg(n):
        return rng.integers(1, 1 << 40, size=n, dtype=np.uint64)

    def plant(name, n, at):
        if all(0 <= a < n for a in at):
            k = bg(n)
            k[list(at)] = BIG
            out.append((f"argmax {name} n={n} at={list(at)}", "argmax", k, None))

    for n in (0, 1, 64, 65, L, L + 1, 3 * L + 5):
        out.append((f"argmax all zero n={n}", "argmax", np.zeros(n, dtype=np.uint64), None))
        for at in sorted({0, n - 1, 63, 64}):
            plant("single", n, (at,))
        plant("two waves", n, (70, L - 3))                  # lanes 70 and L - 3: waves 1 and the last one
        plant("two waves, smaller index in the higher wave", n, (70, L + 3))   # L + 3 is lane 3 of wave 0, 70 lane 6 of wave 1
        plant("one lane", n, (7, 7 + L))
        plant("one lane", n, (0, L))
        plant("one lane three strides", n, (5, 5 + L, 5 + 2 * L))
        plant("second stride", n, (L + 3, 2 * L - 1))       # lane 3 of wave 0 against the last lane of the last wave
        plant("neighbouring waves", n, (63, 64))
    k = np.full(3 * L + 5, 77, dtype=np.uint64)               # every key the same: index 0
    out.append(("argmax all equal", "argmax", k, None))
    return out


@pytest.fixture(scope="module", params=[0, 1], ids=["class0", "class1"])
def ran(request):
    klass = request.param
    L, S = api.block_class(klass)      # as the library was built: the edges follow a build with another lane count
    assert L % 64 == 0 and L >= 128 and S >= L and S & (S - 1) == 0
    rng = np.random.default_rng(4100 + klass)
    cases = _scan_cases(L, rng) + _sort_cases(L, S, klass, rng) + _argmax_cases(L, rng)
    t0 = time.time()
    res = api.selftest_block(klass, [(op, k, v) for _, op, k, v in cases])
    print(f"\n[block primitives] class {klass} ({L} lanes, {S} sort entries): {len(cases)} cases in one call, {time.time() - t0:.2f} s")
    return klass, L, S, cases, res


def _of(ran, op):
    klass, L, S, cases, res = ran
    got = [(c, r) for c, r in zip(cases, res) if c[1] == op]
    assert got
    return L, S, got


def test_scan(ran):
    L, S, got = _of(ran, "scan")
    assert len(got) == 22
    bad = []
    for (name, _, _, v), (out, ret) in got:
        v = np.asarray(v, dtype=np.int64)
        want = np.concatenate([[0], np.cumsum(v, dtype=np.int64)])
        assert want[-1] < 1 << 31
        if not (out.astype(np.int64) == want).all():
            i = int(np.argwhere(out.astype(np.int64) != want)[0][0])
            bad.append(f"{name}: out[{i}] = {out[i]}, want {want[i]}")
        if not (ret.astype(np.int64) == want[-1]).all():
            bad.append(f"{name}: returned {list(ret)} in lanes 0, 63, 64, {L - 1}, want {want[-1]}")
    assert not bad, "\n".join(bad)


def test_sort_kv(ran):
    L, S, got = _of(ran, "sort_kv")
    assert max(len(c[2]) for c, _ in got) > S or ran[0] == 1   # class 0 reaches the in-HBM branch
    bad = []
    for (name, _, k, v), (ok, ov) in got:
        pairs = sorted(zip((int(x) for x in k), (int(x) & 0xFFFFFFFF for x in np.asarray(v, dtype=np.int64))))
        wk = np.array([p[0] for p in pairs], dtype=np.uint64)
        wv = np.array([p[1] for p in pairs], dtype=np.uint32)
        if not ((ok == wk).all() and (ov.view(np.uint32) == wv).all()):
            i = int(np.argwhere((ok != wk) | (ov.view(np.uint32) != wv))[0][0])
            bad.append(f"{name}: entry {i} = ({int(ok[i]):#x}, {int(ov[i])}), want ({int(wk[i]):#x}, {int(np.int32(wv[i]))})")
    assert not bad, "\n".join(bad)


def test_argmax(ran):
    L, S, got = _of(ran, "argmax")
    names = " ".join(c[0] for c, _ in got)
    for must in ("all zero n=0", "two waves n=", "smaller index in the higher wave", "one lane three strides", "second stride", "neighbouring waves"):
        assert must in names, must
    bad = []
    for (name, _, k, _), (gk, gi) in got:
        bk, bi = 0, NONE_IDX
        for i, x in enumerate(int(x) for x in k):
            if x > bk:
                bk, bi = x, i
        if not ((gk == np.uint64(bk)).all() and (gi == bi).all()):
            bad.append(f"{name}: lanes 0, 63, 64, {L - 1} got keys {[int(x) for x in gk]} idx {list(gi)}, want ({bk}, {bi})")
    assert not bad, "\n".join(bad)

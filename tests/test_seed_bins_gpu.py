"""The bins of the row-parallel backward sweeps as the forward seeding kernels fill them (-m gpu).

k_seed_bwd_g works through four lists of task ids, one per group size (16 / 21 / 32 / 64 lanes).  The lists are filled by the forward
kernels' grant step (hip_fm_coop.h persistent_lanes): every task that gets its pool slice goes to the bin dev_fm.h seed_bwd_class names for the
length of its forward list.  arx_selftest_seed_bins runs the seeding stage itself on a runtime of its own and brings home what device memory
holds after every forward launch: each task's list length, the four counters and the four lists.  Asserted per launch: every task with a list
is in exactly one bin, the one the rule names; no task without a list (an empty one, or one whose pool slice overflowed) is in any; a
counter equals the number of tasks the rule sends to its bin; and the launch's list lengths are the restatement's for the same reads.

The reads are a subset of the seed_shapes workload (tests/workloads.py) chosen from the restatement's shapes so that lists of 16 | 17, 21 | 22
and 32 | 33 entries occur, plus one read shorter than the minimum seed length and one of ambiguous bases only, which give no task at all.
Batches of 1, 63, 64 and 65 reads make wavefronts with 1, 63 and 64 askers and one that spills over."""
import os
import tempfile

import numpy as np
import pytest

import seedcheck
import workloads
from arachne_amd import api

pytestmark = pytest.mark.gpu

KNOBS = ("ARX_SEED_BWD2", "ARX_SEED_BWD_MID", "ARX_SEED_GROUP", "ARX_SEED_GRANT", "ARX_SEED_POOL", "ARX_SEED_TASKS", "ARX_SW_SIMPLE", "ARX_SEED_BATCH", "ARX_SEED_CHUNK")
DEFAULT_K = 10
EDGES = (16, 17, 21, 22, 32, 33)
ERR_POOL_OVERFLOW = 4
N_BATCH = 65
EXTRA_AT = (5, 6)      # where the two reads that give no task stand in the batch


def seed_bwd_class(n, mid):
    return -1 if n <= 0 else 0 if n <= 16 else 1 if n <= mid else 2 if n <= 32 else 3


@pytest.fixture(scope="module")
def wl(built):
    import oradrv
    g, flat, lens, kinds = workloads.seed_shapes()
    d = tempfile.mkdtemp(prefix="arx_seed_bins_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    api.index_build(fa, fa)
    o = oradrv.Oracle(fa)
    exp = seedcheck.Expected(o, flat, lens, kf=DEFAULT_K, k3=1)
    # from the restatement alone: reads whose first two passes hold a list of each edge length, then reads with long lists, then the rest in order
    p12, n = exp.col("pass") < 3, exp.col("fwd_n")
    picked = []
    for e in EDGES + (40, 70):
        have = np.unique(exp.shape_read[p12 & ((n == e) if e in EDGES else (n >= e))])
        have = [int(r) for r in have if int(r) not in picked]
        assert have, f"the workload has no list of {e} entries"
        picked.append(have[0])
    picked += [r for r in range(len(lens)) if r not in picked][:N_BATCH - 2 - len(picked)]
    assert len(picked) == N_BATCH - 2
    off = np.concatenate([[0], np.cumsum(lens)])
    reads = [np.asarray(flat[off[r]:off[r + 1]], dtype=np.uint8) for r in picked]
    owner = list(picked)
    for at, extra in zip(EXTRA_AT, (reads[0][:12].copy(), np.full(40, 4, dtype=np.uint8))):   # shorter than the minimum seed length; ambiguous bases only
        reads.insert(at, extra)
        owner.insert(at, -1)
    ref = api.Reference(fa)
    yield ref, exp, reads, owner
    ref.close()
    o.close()


def _want(exp, owner, ps):
    """Sorted list lengths of the pass-`ps` bwt_smem1a calls of the batch's reads (owner: workload index per read, -1: a read that gives no task)."""
    own = np.array([r for r in owner if r >= 0], dtype=np.int64)
    m = (exp.col("pass") == ps) & np.isin(exp.shape_read, own)
    return np.sort(exp.col("fwd_n")[m].astype(np.int64))


def _run(ref, reads, monkeypatch, var):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in var.items():
        monkeypatch.setenv(k, str(v))
    return api.selftest_seed_bins(ref, np.concatenate(reads), np.array([len(r) for r in reads], dtype=np.int32))


def _check_launch(L, mid, what):
    n, t0, task_n = L["n"], L["t0"], L["task_n"].astype(np.int64)
    cls = np.array([seed_bwd_class(int(x), mid) for x in task_n], dtype=np.int64)
    seen = np.zeros(n, dtype=np.int64)
    for c in range(4):
        ids = L["bins"][c].astype(np.int64)
        assert L["cnt"][c] == int((cls == c).sum()), (what, c, L["cnt"], [int((cls == k).sum()) for k in range(4)])
        assert ((ids >= t0) & (ids < t0 + n)).all(), (what, c, "an id outside the launch's tasks")
        assert (cls[ids - t0] == c).all(), (what, c, "a task in a bin the rule does not name")
        np.add.at(seen, ids - t0, 1)
    assert (seen[cls >= 0] == 1).all(), (what, "a task with a list is not in exactly one bin")
    assert (seen[cls < 0] == 0).all(), (what, "a task without a list is in a bin")
    return cls


def test_edge_lengths_occur(wl):
    """From the restatement alone, before the device is looked at: the 65-read batch holds lists either side of every bin edge, in all four bins."""
    ref, exp, reads, owner = wl
    have = set(_want(exp, owner, 1).tolist()) | set(_want(exp, owner, 2).tolist())
    assert set(EDGES) <= have, sorted(have)
    assert max(have) > 64 and min(have) <= 16
    assert len(reads[EXTRA_AT[0]]) < 19 and (reads[EXTRA_AT[1]] == 4).all()


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65])
def test_bins_by_batch_size(wl, monkeypatch, n_reads):
    ref, exp, reads, owner = wl
    out = _run(ref, reads[:n_reads], monkeypatch, {})
    assert len(out) == 2 and all(L["err"] == 0 for L in out), out
    for ps, L in zip((1, 2), out):
        _check_launch(L, 21, f"{n_reads} reads, pass {ps}")
        assert np.array_equal(np.sort(L["task_n"]), _want(exp, owner[:n_reads], ps)), (n_reads, ps)   # the two reads without a seed gave no task
    assert out[0]["t0"] == 0 and out[1]["t0"] == out[0]["n"]
    if n_reads >= 63:
        assert all(out[0]["cnt"][c] + out[1]["cnt"][c] > 0 for c in range(4)), (out[0]["cnt"], out[1]["cnt"])   # all four bins are used


@pytest.mark.parametrize("var", [{"ARX_SEED_GRANT": 1}, {"ARX_SEED_GRANT": 64}, {"ARX_SEED_BWD_MID": 16}], ids=["grant1", "grant64", "mid16"])
def test_bins_by_knob(wl, monkeypatch, var):
    ref, exp, reads, owner = wl
    mid = int(var.get("ARX_SEED_BWD_MID", 21))
    out = _run(ref, reads, monkeypatch, var)
    assert len(out) == 2 and all(L["err"] == 0 for L in out)
    for ps, L in zip((1, 2), out):
        _check_launch(L, mid, f"{var}, pass {ps}")
        assert np.array_equal(np.sort(L["task_n"]), _want(exp, owner, ps))
    if mid == 16:
        w = np.concatenate([_want(exp, owner, 1), _want(exp, owner, 2)])
        assert ((w > 16) & (w <= 21)).any() and out[0]["cnt"][1] == 0 and out[1]["cnt"][1] == 0, out


def test_two_groups(wl, monkeypatch):
    """ARX_SEED_GROUP: the groups of reads go through the same pools and bins one after the other; counters and bins are per group and per pass."""
    ref, exp, reads, owner = wl
    gr = 33
    out = _run(ref, reads, monkeypatch, {"ARX_SEED_GROUP": gr})
    assert len(out) == 4 and all(L["err"] == 0 for L in out)
    for g, (lo, hi) in enumerate(((0, gr), (gr, N_BATCH))):
        for ps in (1, 2):
            L = out[2 * g + ps - 1]
            _check_launch(L, 21, f"group {g}, pass {ps}")
            assert np.array_equal(np.sort(L["task_n"]), _want(exp, owner[lo:hi], ps)), (g, ps)


def test_pool_overflow_tasks_are_in_no_bin(wl, monkeypatch):
    """ARX_SEED_POOL lowered until slices overflow: those tasks keep n = 0, the error bit is raised, and they are in no bin."""
    ref, exp, reads, owner = wl
    hit = False
    for pool in (96, 48, 24):
        out = _run(ref, reads, monkeypatch, {"ARX_SEED_POOL": pool})
        for i, L in enumerate(out):
            cls = _check_launch(L, 21, f"pool {pool}, launch {i}")
            if (L["err"] & ERR_POOL_OVERFLOW) and (cls < 0).any() and (cls >= 0).any():
                hit = True
        if hit:
            assert out[-1]["err"] & ERR_POOL_OVERFLOW
            break
    assert hit, "no pool size made some slices overflow and left others"


def test_other_backward_variants_get_no_bins(wl, monkeypatch):
    """ARX_SEED_BWD2 = 0, 1, 3 and ARX_SW_SIMPLE take the tasks in id order: the forward kernels are given no bins and nothing is recorded."""
    ref, exp, reads, owner = wl
    for var in ({"ARX_SEED_BWD2": 0}, {"ARX_SEED_BWD2": 1}, {"ARX_SEED_BWD2": 3}, {"ARX_SW_SIMPLE": 1}):
        assert _run(ref, reads, monkeypatch, var) == [], var

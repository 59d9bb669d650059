"""Every seeding kernel variant on the GPU against the restatement, interval for interval (-m gpu).

hip_fm_coop.h holds four backward-sweep kernels (k_seed_bwd, k_seed_bwd2, k_seed_bwd_g<FIT32> with 16 / 21 / 32 / 64-lane bodies, k_seed_bwd_e),
the whole-wavefront hand-off k_seed_bwd_wave, text mode's tail, two forward kernels with the table jump, the owed-prefix grant step and text
mode, k_strat_dyn with the k-mer table and two locate forms; which of them runs is decided by what arx_open built and by per-batch knobs.
None of that exists in the host double.  Here each variant runs the seed_shapes workload (tests/workloads.py; what it makes the kernels do is
asserted from the restatement in tests/test_seed_shapes_hostsim.py) and is compared with the restatement's intervals for EVERY read, bit for
bit; variants that change locate are compared chain by chain, seed by seed as well.  The expected values are computed once.

Which path ran is asserted, not assumed: Batch.seed_census() (arx_batch_debug_seed_census, off outside tests) reports per launch the sizes of
the row-parallel kernel's four bins, the tasks flagged for k_seed_bwd_wave and for the tail and the length of the hand-off list -- all of it in
device memory after a launch anyway -- and each variant's counts are checked against the restatement's for the same input
(seedcheck.Expected.census / handed_bounds).

Knobs are read when a context (index knobs) or a batch (all others) is created and at no other time (arachne_amd/csrc/switches.h; DESIGN.md
section 13 is the table of every switch with its read time), so the environment is set before that.  Values the code does
not support are left out: ARX_SEED_BWD_MID takes 16 .. 21 (the 21-lane body holds no longer row), ARX_SEED_BATCH is kept in 8 bits with 0 meaning
the default, ARX_SEED_GRANT 0 means 64.
"""
import os
import tempfile
import time

import numpy as np
import pytest

import seedcheck
import workloads
from arachne_amd import api

pytestmark = pytest.mark.gpu

INDEX_KNOBS = ("ARX_TEXT_INDEX", "ARX_SA_DENSE", "ARX_KMER_K", "ARX_KMER_FWD")
BATCH_KNOBS = ("ARX_SEED_BWD2", "ARX_SEED_FIT32", "ARX_TEXT_BWD", "ARX_SEED_BWD_MID", "ARX_SEED_BWD_BUDGET", "ARX_SEED_GROUP", "ARX_SEED_BPC",
               "ARX_SEED_BWD_BPC", "ARX_STRAT_BPC", "ARX_SEED_CHUNK", "ARX_SEED_BWD_CHUNK", "ARX_SEED_BATCH", "ARX_SEED_BWD_BATCH", "ARX_SEED_GRANT",
               "ARX_SEED_POOL", "ARX_SEED_TASKS", "ARX_SEED_BWD_E_BPC", "ARX_SEED_BWD_E_CHUNK")
DEFAULT_K = 10          # the largest K with 4^K <= the 3.18 M symbols of the workload's text (api_impl.h)
FILE_SA_INTV = 32       # bwa's suffix-array sample, what index_build writes


@pytest.fixture(scope="module")
def wl(built):
    import oradrv
    g, flat, lens, kinds = workloads.seed_shapes()
    d = tempfile.mkdtemp(prefix="arx_seed_variants_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    api.index_build(fa, fa)
    o = oradrv.Oracle(fa)
    exp = seedcheck.Expected(o, flat, lens, kf=DEFAULT_K, k3=1)
    exp.chains()
    yield fa, o, flat, lens, exp
    o.close()


def _setenv(monkeypatch, var):
    for k in INDEX_KNOBS + BATCH_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in var.items():
        monkeypatch.setenv(k, str(v))


def _label(var):
    return ",".join(f"{k[4:]}={v}" for k, v in var.items()) or "default"


def _check_census(cen, exp, var, text, n_reads):
    """What the knobs promise, against the restatement's counts for the same reads."""
    var = {k: str(v) for k, v in var.items()}
    mode = int(var.get("ARX_SEED_BWD2", 2))
    groups = -(-n_reads // int(var.get("ARX_SEED_GROUP", n_reads)))
    assert cen["launches"] == 2 * groups, cen          # first pass + re-seeding, per group of reads
    if mode == 2:
        mid = int(var.get("ARX_SEED_BWD_MID", 21))
        want = exp.census(mid)
        tails = want.pop("to_tail")
        got = {k: cen[k] for k in want}
        assert got == want, (got, want)
        assert cen["wave_list"] == want["to_wave"], cen  # every flagged task reached k_seed_bwd_wave's list
        if mid == 16:
            assert cen["bin21"] == 0
        else:
            assert min(cen["bin16"], cen["bin21"], cen["bin32"], cen["bin64"]) > 0
        assert cen["to_wave"] > 0                       # the branch `k.n > GL` of the 64-lane body
        if text and var.get("ARX_TEXT_BWD") != "0":
            assert cen["to_tail"] == tails and tails > 0, (cen, tails)
        else:
            assert cen["to_tail"] == 0, cen
    elif mode in (0, 1):
        budget = int(var.get("ARX_SEED_BWD_BUDGET", 128))
        assert cen["bin16"] + cen["bin21"] + cen["bin32"] + cen["bin64"] + cen["to_tail"] == 0, cen
        if budget == 0:
            assert cen["wave_list"] == 0, cen
        else:
            lo, hi = exp.handed_bounds(budget)
            assert lo > 0 and lo <= cen["wave_list"] <= hi, (cen, lo, hi)
        if mode == 1:
            assert cen["to_wave"] == cen["wave_list"], cen
    else:
        assert sum(v for k, v in cen.items() if k != "launches") == 0, cen


def _run_variant(ref, flat, lens, exp, monkeypatch, var, text, chains=False):
    _setenv(monkeypatch, var)
    b = ref.batch(flat, lens)
    try:
        b.seed_census(True)
        b.run(api.STAGE_SEED)
        n_iv = exp.check_intervals(b, _label(var))
        cen = b.seed_census()
        _check_census(cen, exp, var, text, len(lens))
        n_ch = None
        if chains:
            b.run(api.STAGE_CHAIN)
            n_ch = exp.check_chains(b, _label(var))
        print(f"  {_label(var):44s} {len(lens)} reads, {n_iv} intervals" + (f", {n_ch} chains" if chains else "") + f" equal; census {cen}")
    finally:
        b.free()


# ---- index variants: one arx_open each
INDEX_VARIANTS = [
    ({}, dict(kmer_k=DEFAULT_K, kmer_fwd_depth=DEFAULT_K, sa_rows_per_entry=1, text_mode=True)),
    ({"ARX_TEXT_INDEX": 0, "ARX_SA_DENSE": 1}, dict(kmer_k=DEFAULT_K, kmer_fwd_depth=DEFAULT_K, sa_rows_per_entry=1, text_mode=False)),
    ({"ARX_TEXT_INDEX": 0}, dict(kmer_k=DEFAULT_K, kmer_fwd_depth=DEFAULT_K, sa_rows_per_entry=4, text_mode=False)),
    ({"ARX_TEXT_INDEX": 0, "ARX_SA_DENSE": 8}, dict(kmer_k=DEFAULT_K, kmer_fwd_depth=DEFAULT_K, sa_rows_per_entry=8, text_mode=False)),
    ({"ARX_TEXT_INDEX": 0, "ARX_SA_DENSE": 32}, dict(kmer_k=DEFAULT_K, kmer_fwd_depth=DEFAULT_K, sa_rows_per_entry=FILE_SA_INTV, text_mode=False)),   # off: k_locate_dyn's longest walks
    ({"ARX_KMER_K": 0}, dict(kmer_k=0, kmer_fwd_depth=0, sa_rows_per_entry=1, text_mode=True)),
    ({"ARX_KMER_K": 4}, dict(kmer_k=4, kmer_fwd_depth=4, sa_rows_per_entry=1, text_mode=True)),
    ({"ARX_KMER_K": 14}, dict(kmer_k=14, kmer_fwd_depth=14, sa_rows_per_entry=1, text_mode=True)),
    ({"ARX_KMER_K": 15}, dict(kmer_k=15, kmer_fwd_depth=14, sa_rows_per_entry=1, text_mode=True)),   # the last level is not part of the forward tables
    ({"ARX_KMER_FWD": 0}, dict(kmer_k=DEFAULT_K, kmer_fwd_depth=0, sa_rows_per_entry=1, text_mode=True)),
    ({"ARX_KMER_K": 14, "ARX_TEXT_INDEX": 0}, dict(kmer_k=14, kmer_fwd_depth=14, sa_rows_per_entry=4, text_mode=False)),
]


@pytest.mark.parametrize("var,info_want", INDEX_VARIANTS, ids=[_label(v) for v, _ in INDEX_VARIANTS])
def test_index_variant(wl, monkeypatch, var, info_want):
    fa, o, flat, lens, exp = wl
    _setenv(monkeypatch, var)
    t0 = time.time()
    ref = api.Reference(fa)
    try:
        info = ref.index_info()
        assert {k: info[k] for k in info_want} == info_want, info
        print(f"\nindex {_label(var)}: {info} (arx_open {time.time() - t0:.2f} s)")
        _run_variant(ref, flat, lens, exp, monkeypatch, var, info["text_mode"], chains=True)
    finally:
        ref.close()


def test_default_variant_equals_compiled_reference(wl, monkeypatch):
    """Where the reference's own C core was compiled (oracle/_ref), the default variant's intervals are compared with its mem_collect_intv
    directly; elsewhere the restatement stands in for it (tests/test_oracle_vs_ref.py pins the two to each other)."""
    import refdrv
    fa, o, flat, lens, exp = wl
    _setenv(monkeypatch, {})
    ref = api.Reference(fa)
    try:
        b = ref.batch(flat, lens).run(api.STAGE_SEED)
        n, iv = b.debug_intv()
        b.free()
    finally:
        ref.close()
    assert np.array_equal(n, exp.n)
    if not refdrv.available():
        print("\n(no compiled reference here: compared with the restatement only)")
        return
    r = refdrv.Ref(fa)
    total = 0
    for i in range(len(lens)):
        want = r.collect_intv(exp.flat[exp.off[i]:exp.off[i + 1]]) if lens[i] >= 19 else np.zeros((0, 4), dtype=np.uint64)
        assert n[i] == len(want) and (iv[i, :n[i]] == want).all(), i
        total += len(want)
    r.close()
    print(f"\ndefault variant: {total} intervals of {len(lens)} reads equal the compiled reference's")


# ---- batch variants; the ones marked True also run without text mode (ARX_TEXT_INDEX=0), where every sweep is walked to its end
def _batch_variants(n_reads):
    return [
        ({"ARX_SEED_BWD2": 0}, True), ({"ARX_SEED_BWD2": 1}, True), ({"ARX_SEED_BWD2": 2}, True), ({"ARX_SEED_BWD2": 3}, True),
        ({"ARX_SEED_FIT32": 0}, True),
        ({"ARX_TEXT_BWD": 0}, False),
        ({"ARX_SEED_BWD_MID": 16}, False), ({"ARX_SEED_BWD_MID": 21}, False),
        ({"ARX_SEED_BWD_BUDGET": 0, "ARX_SEED_BWD2": 0}, False), ({"ARX_SEED_BWD_BUDGET": 8, "ARX_SEED_BWD2": 0}, False),
        ({"ARX_SEED_BWD_BUDGET": 0, "ARX_SEED_BWD2": 1}, False), ({"ARX_SEED_BWD_BUDGET": 8, "ARX_SEED_BWD2": 1}, False),
        ({"ARX_SEED_GROUP": n_reads // 3}, False),
        ({"ARX_SEED_BPC": 1, "ARX_SEED_BWD_BPC": 1, "ARX_STRAT_BPC": 1}, False),              # few wavefronts: every lane refills many times
        ({"ARX_SEED_BPC": 1, "ARX_SEED_BWD2": 0}, False), ({"ARX_SEED_BPC": 1, "ARX_SEED_BWD2": 1}, False),
        ({"ARX_SEED_CHUNK": 1}, False), ({"ARX_SEED_CHUNK": 7}, False),
        ({"ARX_SEED_CHUNK": 1, "ARX_SEED_BWD2": 0}, False), ({"ARX_SEED_CHUNK": 7, "ARX_SEED_BWD2": 1}, False),
        ({"ARX_SEED_BATCH": 1}, False), ({"ARX_SEED_BATCH": 64}, False),
        ({"ARX_SEED_BATCH": 1, "ARX_SEED_BWD2": 0}, False), ({"ARX_SEED_BATCH": 64, "ARX_SEED_BWD2": 0}, False),
        ({"ARX_SEED_GRANT": 1}, False), ({"ARX_SEED_GRANT": 64}, False),
    ]


@pytest.mark.parametrize("text", [True, False], ids=["text_mode", "no_text_index"])
def test_batch_variants(wl, monkeypatch, text):
    fa, o, flat, lens, exp = wl
    _setenv(monkeypatch, {} if text else {"ARX_TEXT_INDEX": 0})
    ref = api.Reference(fa)
    try:
        assert ref.index_info()["text_mode"] == text
        print(f"\nbatch variants, text mode {'on' if text else 'off'}:")
        n, failed = 0, []
        for var, both in _batch_variants(len(lens)):
            if text or both:
                try:
                    _run_variant(ref, flat, lens, exp, monkeypatch, var, text, chains=False)
                except AssertionError as e:       # (a wrong result, not a fault: the other variants still say which kernels are affected)
                    print(f"  {_label(var):44s} FAILED: {str(e)[:300]}")
                    failed.append(_label(var))
                n += 1
        assert not failed, failed
        assert n == (len(_batch_variants(len(lens))) if text else 5)
    finally:
        ref.close()


def test_capped_batch_reset_and_halves(wl, monkeypatch):
    """The same reads cut to 150 bases (the kernels' LDS row is sized by the longest read), the same batch twice in one handle, and the batch in
    two halves through one handle: results do not depend on what ran before or beside."""
    fa, o, flat, lens, exp = wl
    _setenv(monkeypatch, {})
    ref = api.Reference(fa)
    try:
        b = ref.batch(flat, lens)
        b.seed_census(True)
        b.run(api.STAGE_SEED)
        exp.check_intervals(b, "first run")
        b.reset(flat, lens)
        b.run(api.STAGE_SEED)
        exp.check_intervals(b, "same reads again in the same handle")
        cen = b.seed_census(True)
        want = exp.census()
        assert cen["launches"] == 4 and all(cen[k] == 2 * want[k] for k in want), (cen, want)
        half = (len(lens) // 4) * 2
        for name, reads in (("first half", np.arange(0, half)), ("second half", np.arange(half, len(lens)))):
            e = exp.subset(reads)
            b.reset(e.flat, e.lens)
            b.run(api.STAGE_SEED)
            e.check_intervals(b, name)
            cen = b.seed_census(True)
            want = e.census()
            assert all(cen[k] == want[k] for k in want), (name, cen, want)
        b.free()
        g, cflat, clens, _ = workloads.seed_shapes(cap=150)
        cexp = seedcheck.Expected(o, cflat, clens, kf=DEFAULT_K, k3=1)
        assert max(cexp.coverage()["list_lengths_swept"]) > 64
        for var in ({}, {"ARX_SEED_BWD2": 0}, {"ARX_SEED_BWD2": 1}, {"ARX_SEED_BWD2": 3}):
            _run_variant(ref, cflat, clens, cexp, monkeypatch, var, True)
    finally:
        ref.close()


@pytest.mark.parametrize("knob,values", [("ARX_SEED_POOL", (384, 256, 128, 64, 24, 6)), ("ARX_SEED_TASKS", (12, 8, 5, 3, 2, 1))])
def test_pool_and_task_limits_are_never_silent(wl, monkeypatch, knob, values):
    """The interval pool and the task array are sized per read; a batch that does not fit is reported (ERR_POOL_OVERFLOW through arx_last_error),
    never answered with fewer intervals.  Stepped down from the default: every run either raises or gives exactly the restatement's intervals."""
    fa, o, flat, lens, exp = wl
    _setenv(monkeypatch, {})
    ref = api.Reference(fa)
    try:
        outcome = {}
        for v in values:
            _setenv(monkeypatch, {knob: v})
            b = ref.batch(flat, lens)
            try:
                b.run(api.STAGE_SEED)
                exp.check_intervals(b, f"{knob}={v}")
                outcome[v] = "equal"
            except api.ArachneError as e:
                assert "error bits" in str(e), e
                outcome[v] = "raised"
            finally:
                b.free()
        print(f"\n{knob}: {outcome}")
        assert outcome[values[0]] == "equal" and outcome[values[-1]] == "raised", outcome
        seen = [outcome[v] for v in values]
        assert seen == sorted(seen), outcome            # once it raises it keeps raising as the limit shrinks
    finally:
        ref.close()

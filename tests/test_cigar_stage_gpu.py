"""The CIGAR stage itself on the GPU (-m gpu), on the planted cases of tests/cigarcases.py.

arx_selftest_reg2aln runs Pipeline<HipRT>::stage_reg2aln -- the classification by the first band, k_reg2aln_nw_g16 per band class with its band
retries, the <1,16> launch that takes what the class kernels hand on, the one-thread path for long regions, the slot loop and compact() -- on
region rows the test made up.  Every Aln field parity.ALN_MAP names, the CIGAR offset and every CIGAR word are compared bit for bit with the
restatement's ora_reg2aln (and, for the default variant, with the compiled reference's mem_reg2aln where oracle/_ref is present); the census the
entry brings home is compared exactly with the counts the restatement's shape rows give: regions per band class, gap-free regions finished
inline, long regions, punts, passes of the slot loop and the final slot width; and every queued region's slice of traceback matrix must hold the
rows of its widest executed try.  That the cases reach the edges they are named after is asserted on the CPU (tests/test_cigar_cases_hostsim.py)."""
import os
import shutil

import numpy as np
import pytest

import cigarcases as cc
import parity
from arachne_amd import api

pytestmark = pytest.mark.gpu

KNOBS = ("ARX_SW_SIMPLE", "ARX_COOP_BPC", "ARX_BPC")
assert {n for n, _ in parity.ALN_MAP} <= {n for n, _ in cc.ALN_COLS}


@pytest.fixture(scope="module")
def cases(built):
    import oradrv
    c = {}
    for name, b in (("main", cc.build_main()), ("small", cc.build_small())):
        fa = cc.write_index(b)
        o = oradrv.Oracle(fa)
        flat = cc.flatten(b)
        c[name], c[name + "_fa"], c[name + "_flat"], c[name + "_exp"] = b, fa, flat, cc.expected(o, flat)
        o.close()
        c[name + "_ref"] = api.Reference(fa)
    yield c
    c["main_ref"].close()
    c["small_ref"].close()
    for name in ("main", "small"):
        shutil.rmtree(os.path.dirname(c[name + "_fa"]), ignore_errors=True)


def _run(ref, flat, monkeypatch, env=None, census=True, grid_cap=0):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return api.selftest_reg2aln(ref, flat["seqs"], flat["lens"], flat["cap"], flat["n_regs"], flat["regs"], census=census, grid_cap=grid_cap)


def test_default(cases, monkeypatch):
    flat, exp = cases["main_flat"], cases["main_exp"]
    dev = _run(cases["main_ref"], flat, monkeypatch)
    assert dev["err"] == 0
    cc.check_stage(dev, flat, exp)
    assert dev["census"]["known"] == 0x7ff
    want = cc.check_census(dev["census"], flat, exp["shapes"], passes=3, cig_w=64)
    assert dev["census"]["punts"] >= 20
    cc.check_slices(dev["census"], want)


def test_default_against_the_compiled_reference(cases, monkeypatch):
    import refdrv
    refdrv.need("ref_reg2aln")
    flat = cases["main_flat"]
    r = refdrv.Ref(cases["main_fa"])
    try:
        ref = cc.expected(r, flat, with_shape=False)
    finally:
        r.close()
    cc.check_stage(_run(cases["main_ref"], flat, monkeypatch, census=False), flat, ref)


def test_one_thread_form(cases, monkeypatch):
    """ARX_SW_SIMPLE: every queued region on the serial reg2aln of dev_regs.h (no punt list: the census says so)."""
    flat, exp = cases["main_flat"], cases["main_exp"]
    dev = _run(cases["main_ref"], flat, monkeypatch, {"ARX_SW_SIMPLE": "1"})
    assert dev["err"] == 0
    cc.check_stage(dev, flat, exp)
    assert dev["census"]["punts"] == -1 and not dev["census"]["known"] >> 9 & 1
    cc.check_census(dev["census"], flat, exp["shapes"], passes=3, cig_w=64, punts=False)


def test_coop_bpc_1(cases, monkeypatch):
    """ARX_COOP_BPC=1: one workgroup per compute unit for the class launches (at this batch's size that is still a group per region)."""
    flat, exp = cases["main_flat"], cases["main_exp"]
    dev = _run(cases["main_ref"], flat, monkeypatch, {"ARX_COOP_BPC": "1"})
    assert dev["err"] == 0
    cc.check_stage(dev, flat, exp)
    cc.check_census(dev["census"], flat, exp["shapes"], passes=3, cig_w=64)


@pytest.mark.parametrize("blocks", [1, 2])
def test_grid_far_smaller_than_the_class_lists(cases, monkeypatch, blocks):
    """One or two workgroups per class launch and two for what they hand on: each 16-lane group walks its grid-stride loop through many regions of
    one class, one after the other through the same LDS rows (four groups per workgroup: 4 x blocks regions in flight)."""
    flat, exp = cases["main_flat"], cases["main_exp"]
    dev = _run(cases["main_ref"], flat, monkeypatch, grid_cap=blocks)
    assert dev["err"] == 0
    cen = dev["census"]
    assert max(cen["per_class"]) > 10 * 4 * blocks and sorted(cen["per_class"])[1] > 4 * blocks, cen["per_class"]   # four of the five lists take several trips ...
    assert cen["punts"] > 3 * 4 * 2                                                                                   # ... and so does the launch behind them
    cc.check_stage(dev, flat, exp)
    want = cc.check_census(cen, flat, exp["shapes"], passes=3, cig_w=64)
    cc.check_slices(cen, want)


def test_two_halves(cases, monkeypatch):
    b, exp = cases["main"], cases["main_exp"]
    h = len(b.reads) // 2
    parts = [cc.flatten(b, range(0, h)), cc.flatten(b, range(h, len(b.reads)))]
    devs = [_run(cases["main_ref"], p, monkeypatch, census=False) for p in parts]
    n0 = int(devs[0]["reg_off"][-1])
    alns = np.concatenate([d["alns"] for d in devs])
    alns["cigar_off"][n0:] += len(devs[0]["cigars"])
    both = dict(reg_off=np.concatenate([devs[0]["reg_off"], devs[1]["reg_off"][1:] + n0]), alns=alns, cigars=np.concatenate([d["cigars"] for d in devs]))
    cc.check_stage(both, cases["main_flat"], exp)


def test_without_the_slot_overflow_cases(cases, monkeypatch):
    """One pass at 16 words, and the regions both batches hold come out as in the batch that went through three passes: the retry leaves nothing stale."""
    flat, exp = cases["main_flat"], cases["main_exp"]
    sub = cc.flatten(cases["main"], cc.reads_without_overflow(flat, exp["shapes"]))
    sexp = cc.subset(flat, exp, sub)
    dev = _run(cases["main_ref"], sub, monkeypatch)
    assert dev["err"] == 0
    cc.check_stage(dev, sub, sexp)
    cc.check_census(dev["census"], sub, sexp["shapes"], passes=1, cig_w=16)


def test_pool_overflow_and_short_class_lists(cases, monkeypatch):
    """The call of its own: class lists of 1, 3, 4 and 5 regions, no punt, and one long region whose matrix the one-thread path cannot hold --
    ERR_POOL_OVERFLOW in the error word, that region refused (rid -1, no CIGAR), every other region exact."""
    flat, exp = cases["small_flat"], cases["small_exp"]
    dev = _run(cases["small_ref"], flat, monkeypatch)
    assert dev["err"] == cc.ERR_POOL_OVERFLOW
    cc.check_stage(dev, flat, exp, skip=[flat["tags"].index("beyond z_cap")])
    want = cc.check_census(dev["census"], flat, exp["shapes"], passes=1, cig_w=16)
    assert dev["census"]["per_class"][:4] == [1, 3, 4, 5] and dev["census"]["punts"] == 0 and dev["census"]["big"] == 2
    cc.check_slices(dev["census"], want)


@pytest.mark.parametrize("case", [t for t, _, _ in cc.SLOT_CASES])
def test_slot_case_alone(cases, monkeypatch, case):
    """16 words exactly (14 operations and both clips, or a squeezed leading deletion) cost no retry, 15 operations cost one, 30 stop at 32 words,
    31 reach 64: each read in a batch of its own, on either strand."""
    for tag, sub, sexp, passes, cig_w in cc.slot_batches(cases["main"], cases["main_flat"], cases["main_exp"], only=case):
        dev = _run(cases["main_ref"], sub, monkeypatch)
        assert dev["err"] == 0, tag
        cc.check_stage(dev, sub, sexp)
        cc.check_census(dev["census"], sub, sexp["shapes"], passes=passes, cig_w=cig_w)

"""The three DP kernel families driven directly (include/arachne_amd.h: arx_selftest_extend / arx_selftest_rescue_sw / arx_selftest_gen_cigar)
and compared field by field, bit for bit, with the oracle:
  extension   every variant of HipRT::run_extend -- one launch per query-length class (k_extend_b16<C>), the merged launch
              (k_extend_classes_b), round 2's kernel (ext2_g16), the one-thread form (ext2_task) -- against ksw_extend2(q, t, w, 5, 100, h0),
              also with a grid far smaller than the task count;
  rescue SW   k_sw_u8_g16<SL> for SL = 10 / 16 / 32 (the byte form and, for mates of 250+ bases, the i16 form), with and without the pre-filter
              k_sw_filter_g16, and the one-thread form, against ksw_align2(revcomp(mate), window, XSUBO|XSTART|(XBYTE iff l_ms < 250)|19);
  CIGAR       gen_cigar2_g16<LO,HI> of each band class kernel and of the <1,16> punt kernel against ksw_global2(q, t, w) with bwa_gen_cigar2's
              band (the gap-free shortcut by its own sum), NM by bwa.c's rule; "punted" exactly when n_col > 16 * HI.
The compiled reference's own vectors (tests/golden, the cases with the path's parameters) run first through every variant; then the seeded
cases of tests/dpcases.py, whose coverage tests/test_dp_cases_hostsim.py asserts.  Contracts of the entries: see that module's docstring."""
import os
import tempfile

import numpy as np
import pytest

import __graft_entry__ as ge
import dpcases
import oradrv
import workloads
from arachne_amd import api

pytestmark = pytest.mark.gpu
SEED = 20261016


@pytest.fixture(scope="module")
def env(built):
    ge.build_product()
    z = np.load(os.path.join(workloads.GOLDEN_DIR, "bwa_path_v1.npz"))
    o = oradrv.Oracle(workloads.unpack_index(z, tempfile.mkdtemp(prefix="arx_dpk_")))
    return z, o


def _diff(got, exp, cases, what):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    return [(what, int(i), cases[i]["kind"], got[i].tolist(), exp[i].tolist()) for i in bad[:5]], len(bad)


@pytest.fixture(scope="module")
def ext(env):
    z, o = env
    cases = dpcases.ext_cases(SEED, golden=z)
    text, bases, tasks = dpcases.ext_layout(cases, SEED)
    return cases, text, bases, tasks, dpcases.ext_oracle(o, cases)


@pytest.mark.parametrize("mode,grid_cap", [(0, 0), (1, 0), (2, 0), (3, 0), (0, 3), (1, 5), (3, 2)])
def test_extension_kernels(ext, mode, grid_cap):
    cases, text, bases, tasks, exp = ext
    gold = np.array([c["kind"] == "golden" for c in cases])
    got = api.selftest_extend(text.pac, text.l_pac, bases, tasks, mode=mode, grid_cap=grid_cap)
    first, n_bad = _diff(got[gold], exp[gold], [c for c in cases if c["kind"] == "golden"], "golden")
    assert n_bad == 0, first
    first, n_bad = _diff(got, exp, cases, "generated")
    assert n_bad == 0, (n_bad, first)
    print(f"extension mode {mode} grid_cap {grid_cap}: {len(cases)} cases ({int(gold.sum())} golden) bit-identical, classes {dpcases.ext_coverage(cases, exp)['per_class']}")


@pytest.fixture(scope="module")
def sw(env):
    z, o = env
    cases = dpcases.sw_cases(SEED, golden=z)
    return cases, dpcases.sw_oracle(o, cases)


@pytest.mark.parametrize("max_len,filt,simple,grid_cap", [(160, 0, 0, 0), (249, 0, 0, 0), (255, 0, 0, 0), (160, 1, 0, 0), (255, 1, 0, 0),
                                                          (255, 0, 1, 0), (255, 0, 0, 3), (249, 1, 0, 2)])
def test_rescue_sw_kernels(sw, max_len, filt, simple, grid_cap):
    cases_all, exp_all = sw
    keep = [i for i, c in enumerate(cases_all) if len(c["mate"]) <= max_len]   # a launch holds the mates its max_len allows (SL 10: <= 160, ...)
    cases, exp = [cases_all[i] for i in keep], exp_all[keep]
    text, mates, mo, ml, win = dpcases.sw_layout(cases, SEED)
    got = api.selftest_rescue_sw(text.pac, text.l_pac, mates, mo, ml, win, max_len, filter=bool(filt), sw_simple=bool(simple), grid_cap=grid_cap)
    dropped = (got == dpcases.NONE_U8).all(axis=1) & (exp != dpcases.NONE_U8).any(axis=1)
    if filt:      # a task the pre-filter drops gets the "none" record; ksw_align2 must then stay below min_seed_len
        assert (exp[dropped, 0] < dpcases.MIN_SEED_LEN).all(), [(int(i), exp[i].tolist()) for i in np.nonzero(dropped & (exp[:, 0] >= dpcases.MIN_SEED_LEN))[0][:5]]
        assert dropped.sum() > 50
    else:
        assert not dropped.any()
    keep2 = ~dropped
    first, n_bad = _diff(got[keep2], exp[keep2], [c for c, k in zip(cases, keep2) if k], "sw")
    assert n_bad == 0, (n_bad, first)
    n_gold = sum(1 for c in cases if c["kind"] == "golden")
    print(f"rescue max_len {max_len} filter {filt} simple {simple} grid_cap {grid_cap}: {len(cases)} cases ({n_gold} golden), {int(dropped.sum())} dropped, "
          f"{int(keep2.sum())} bit-identical, {sum(1 for c in cases if len(c['mate']) >= 250)} in the i16 form")


@pytest.fixture(scope="module")
def nw(env):
    z, o = env
    cases = dpcases.nw_cases(SEED, golden=z)
    return cases, [dpcases.nw_oracle(o, c) for c in cases]


@pytest.mark.parametrize("klass", [0, 1, 2, 3, 4, 5])
def test_cigar_kernels(nw, klass):
    cases, exp = nw
    cap = np.array([c["cap"] for c in cases], dtype=np.int32)
    out, cig = api.selftest_gen_cigar([c["q"] for c in cases], [c["t"] for c in cases], [c["w_"] for c in cases], klass, cap=cap, cig_w=1024)
    n_run = n_punt = n_gold = 0
    bad = []
    for i, (c, (sc, cg, nm)) in enumerate(zip(cases, exp)):
        shortcut = len(c["q"]) == len(c["t"]) and c["w_"] == 0
        n_col = dpcases.gen_cigar_band(len(c["q"]), len(c["t"]), c["w_"])[1]
        want_punt = not shortcut and n_col > 16 * dpcases.NW_HI[klass]
        if out[i, 3] != int(want_punt):
            bad.append((i, c["kind"], "punted", int(out[i, 3]), want_punt))
            continue
        if want_punt:
            n_punt += 1
            continue
        n_run += 1
        n_gold += c["kind"] == "golden"
        ok = out[i, 0] == sc and out[i, 1] == len(cg) and out[i, 2] == nm
        if ok and len(cg) <= c["cap"]:
            ok = (cig[i, :len(cg)] == cg).all()
        if not ok:
            bad.append((i, c["kind"], out[i].tolist(), (sc, len(cg), nm)))
    assert not bad, (len(bad), bad[:5])
    assert n_run > 300
    print(f"CIGAR kernel {klass}: {n_run} cases bit-identical ({n_gold} golden), {n_punt} punted")

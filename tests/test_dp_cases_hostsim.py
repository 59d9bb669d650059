"""The DP case generator of tests/dpcases.py on the CPU: the serial forms of the host test double (dev_sw.h ext2_task and u8_align, what the
one-thread ARX_SW_SIMPLE path runs) against the oracle's ksw_extend2 / ksw_align2, and the CIGAR cases' oracle answers against the
compiled reference's own vectors.  This checks the generator, the text layout (.pac, doubled coordinates, both strands and directions) and
the comparison code without a GPU, and asserts that the cases reach the edges tests/test_dp_kernels_gpu.py runs the kernels at.

Contracts of the self-test entries (include/arachne_amd.h), as the pipeline guarantees them:
  extension  1 <= qlen <= 255 (MAX_READ_LEN: the 16-lane tilings hold 16 * C > qlen columns), the target on one strand of [0, 2 l_pac),
             w >= 1, 1 <= h0 <= 255 (a seed or left-extension score of a read of at most 255 bases);
  rescue     1 <= l_ms <= max_len <= 255, 1 <= tlen <= SW_T_CAP = 800 (the LDS rows of the kernel; PES_HIGH - PES_LOW + 255 = 790 at most);
  CIGAR      1 <= qlen <= NW_Q_CAP = 256, 1 <= tlen <= NW_T_CAP = 1024 (the LDS staging of k_reg2aln_nw_g16), w_ >= 0, cap >= 1."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dpcases
import oradrv
import workloads

SIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "libarx_hostsim.so")
SEED = 20261016


@pytest.fixture(scope="module")
def env(built):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    sim = C.CDLL(SIM)
    sim.arx_test_ext2_task.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    sim.arx_test_sw_exact_f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    sim.arx_test_sw_prefilter.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    z = np.load(os.path.join(workloads.GOLDEN_DIR, "bwa_path_v1.npz"))
    o = oradrv.Oracle(workloads.unpack_index(z, tempfile.mkdtemp(prefix="arx_dpc_")))      # any index: the DP entries only need the scoring matrix
    return sim, z, o


def test_text_layout_reads_back_every_target():
    rng = np.random.default_rng(3)
    text = dpcases.Text(rng)
    ts = [dpcases.rand_seq(rng, rng.integers(1, 40)) for _ in range(64)]
    hs = [(text.add(t, k % 2, 1 if k % 4 < 2 else -1), k % 2, 1 if k % 4 < 2 else -1) for k, t in enumerate(ts)]
    text.finish()
    for t, (h, strand, tdir) in zip(ts, hs):
        p = text.pos[h]
        got = [text.base(p + i * tdir) for i in range(len(t))]
        assert got == t.tolist()
        assert (p >= text.l_pac) == (strand == 1) and (p + (len(t) - 1) * tdir >= text.l_pac) == (strand == 1)


def test_serial_extension_on_the_generated_cases(env):
    sim, z, o = env
    cases = dpcases.ext_cases(SEED, golden=z)
    text, bases, tasks = dpcases.ext_layout(cases, SEED)
    got = np.zeros((len(cases), 6), dtype=np.int32)
    sim.arx_test_ext2_task(text.pac.ctypes.data, text.l_pac, bases.ctypes.data, len(cases), tasks.ctypes.data, got.ctypes.data)
    exp = dpcases.ext_oracle(o, cases)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, [(int(i), cases[i]["kind"], got[i].tolist(), exp[i].tolist()) for i in bad[:5]]
    gold = [i for i, c in enumerate(cases) if c["kind"] == "golden"]
    assert len(gold) > 150
    cov = dpcases.ext_coverage(cases, exp)
    assert min(cov["per_class"]) >= 60, cov
    assert cov["qlen_edges"] == sorted(dpcases.QLEN_EDGES), cov
    assert cov["tlen_0"] >= 40 and cov["tlen_0_classes"] == list(range(7)) and cov["tlen_2_3"] >= 80, cov
    assert cov["tlen_1"] >= 20 and cov["tlen_511_513"] == [511, 512, 513] and cov["tlen_over_512"] >= 60, cov
    assert cov["both_dirs_strands"] == 8, cov
    assert cov["w_100"] > 300 and cov["w_200"] > 200 and cov["w_small"] >= 100 and cov["w_over_qlen"] >= 150, cov
    assert cov["h0_over_200_short_q"] >= 20 and cov["n_in_query"] >= 80, cov
    assert cov["gscore_neg"] >= 100 and cov["gtle_below_tlen"] >= 500 and cov["max_off_half_w"] >= 15, cov
    assert cov["score_h0_only"] >= 30 and cov["stopped_early"] >= 150, cov


def test_serial_rescue_sw_on_the_generated_cases(env):
    sim, z, o = env
    cases = dpcases.sw_cases(SEED, golden=z)
    exp = dpcases.sw_oracle(o, cases)
    n_dropped = 0
    for i, c in enumerate(cases):
        q = dpcases.revcomp(c["mate"])
        got = np.zeros(7, dtype=np.int32)
        sim.arx_test_sw_exact_f(q.ctypes.data, len(q), c["t"].ctypes.data, len(c["t"]), dpcases.sw_xtra(len(q)), 1, got.ctypes.data)
        assert (got == exp[i]).all(), (i, c["kind"], got.tolist(), exp[i].tolist())
        if not sim.arx_test_sw_prefilter(q.ctypes.data, len(q), c["t"].ctypes.data, len(c["t"])):
            assert exp[i][0] < dpcases.MIN_SEED_LEN, (i, exp[i].tolist())
            n_dropped += 1
    assert sum(1 for c in cases if c["kind"] == "golden") > 200
    cov = dpcases.sw_coverage(cases, exp)
    assert len(cov["mates_16k_edges"]) == 18 and cov["mates_160_161"] == [160, 161] and cov["mates_249_255"] == [249, 250, 255], cov
    assert cov["i16"] >= 40 and cov["odd_tlen"] >= 300 and cov["tlen_below_qlen"] >= 100 and cov["tlen_784_800"] == [784, 800], cov
    assert cov["score_18"] >= 15 and cov["score_19"] >= 15 and cov["score_20"] >= 15, cov
    assert cov["score2_eq_score"] >= 50 and cov["tb_qb_set"] >= 500 and cov["reverse_strand"] >= 500 and cov["n_in_mate"] >= 60, cov
    assert n_dropped >= 100


def test_cigar_cases_and_their_oracle(env):
    sim, z, o = env
    cases = dpcases.nw_cases(SEED, golden=z)
    exp = [dpcases.nw_oracle(o, c) for c in cases]
    gold = [(c, e) for c, e in zip(cases, exp) if c["kind"] == "golden"]
    assert len(gold) > 150
    for c, (sc, cg, nm) in gold:                     # the band formula and the oracle give the compiled reference's answers
        assert sc == c["gold"][0] and (cg == c["gold"][1]).all()
    for c, (sc, cg, nm) in zip(cases, exp):         # a CIGAR spans both sequences
        if c["kind"] == "cap":
            continue
        ops = [(int(x) & 0xf, int(x) >> 4) for x in cg]
        assert sum(ln for op, ln in ops if op in (0, 1)) == len(c["q"]) and sum(ln for op, ln in ops if op in (0, 2)) == len(c["t"])
    cov = dpcases.nw_coverage(cases, exp)
    assert min(cov["per_tiling"].values()) >= 30, cov
    assert cov["punts_per_kernel"][:3] >= [300, 200, 60] and cov["punts_per_kernel"][3:] == [0, 0, 0], cov   # n_col <= qlen <= 256 = 16 * 16
    assert cov["gapfree_shortcut"] >= 60 and cov["lead_indel"] >= 40 and cov["trail_indel"] >= 40, cov
    assert cov["n_in_query"] >= 40 and cov["nm_minus1"] >= 40 and cov["tlen_over_512"] >= 40, cov


def test_selftest_entries_refuse_input_outside_the_contract(built):
    """checked on the host before anything touches a device: ARX_E_ARG (-2), so no GPU is needed here"""
    import __graft_entry__ as ge
    from arachne_amd import api
    ge.build_product()
    rng = np.random.default_rng(5)
    text = dpcases.Text(rng)
    h = text.add(dpcases.rand_seq(rng, 600), 0, 1)
    text.finish()
    p, L = text.pos[h], text.l_pac
    q = dpcases.rand_seq(rng, 300)
    ok_ext = [p, 0, 100, 50, 1, 1, 100, 30]
    bad_ext = [dict(), dict(qlen=256), dict(qlen=0), dict(h0=0), dict(h0=256), dict(w=0), dict(tlen=-1), dict(qdir=0), dict(tdir=2),
               dict(tpos=L - 10, tlen=20), dict(tpos=2 * L - 5, tlen=10), dict(tpos=5, tdir=-1, tlen=10), dict(qoff=250, qlen=60)]
    keys = ["tpos", "qoff", "qlen", "tlen", "qdir", "tdir", "w", "h0"]
    for k, d in enumerate(bad_ext):
        row = [d.get(n, v) for n, v in zip(keys, ok_ext)]
        if k == 0:
            continue                                     # (the valid row itself would need a device)
        with pytest.raises(api.ArachneError, match="code -2"):
            api.selftest_extend(text.pac, L, q, np.array([ok_ext, row], dtype=np.int64))
    ok_win = [p, p + 100]
    for ml, win, max_len in ((256, ok_win, 255), (200, ok_win, 160), (0, ok_win, 255), (100, [p, p + 801], 255), (100, [p, p], 255),
                             (100, [L - 50, L + 50], 255), (100, [2 * L - 10, 2 * L + 10], 255)):
        mates = dpcases.rand_seq(rng, 300)
        with pytest.raises(api.ArachneError, match="code -2"):
            api.selftest_rescue_sw(text.pac, L, mates, [0], [ml], [win], max_len)
    for ql, tl, w, cap, klass in ((257, 100, 10, 10, 0), (0, 100, 10, 10, 0), (100, 1025, 10, 10, 0), (100, 0, 10, 10, 0), (100, 100, -1, 10, 0),
                                  (100, 100, 10, 0, 0), (100, 100, 10, 2000, 0), (100, 100, 10, 10, 6)):
        with pytest.raises(api.ArachneError, match="code -2"):
            api.selftest_gen_cigar([dpcases.rand_seq(rng, ql)], [dpcases.rand_seq(rng, tl)], [w], klass, cap=[cap], cig_w=1024)

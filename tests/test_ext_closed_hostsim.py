"""The extensions their diagonal decides (dev_sw.h ext_closed_form, used by KExtStep; ARX_EXT_CLOSED=0 switches it off), on the CPU:
the closed form against ext2_task task by task, and the whole path through the host-compiled test double with the switch on and off."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import parity
import workloads
from arachne_amd import api
from extclosed import assert_same_results, bench_like_inputs, run_both_ways

SIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "libarx_hostsim.so")
GOLD = os.path.join(workloads.GOLDEN_DIR, "bwa_path_v1.npz")


def test_closed_form_equals_the_dp_on_every_accepted_task():
    """Every accepted task's six fields against ext2_task; every task of the grid that its construction makes acceptable is accepted (so the
    entry cannot pass by declining) and no other is; the word-wise walk against the pair-by-pair one.  Grid: see arx_test_ext_closed (tests/hostsim/ext_closed.cpp)."""
    so = os.path.join(tempfile.mkdtemp(prefix="arx_extc_unit_"), "libarx_ext_closed.so")   # dev_sw.h for the host, on its own
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-o", so, os.path.join(os.path.dirname(SIM), "ext_closed.cpp")])
    lib = C.CDLL(so)
    lib.arx_test_ext_closed.restype = C.c_long
    lib.arx_test_ext_closed.argtypes = [C.c_uint, C.c_int, C.POINTER(C.c_long)]
    for seed in (1, 2):
        out = (C.c_long * 6)()
        n = lib.arx_test_ext_closed(seed, 30000, out)
        tasks, should, accepted, wrong, disagree, forms = list(out)
        print("seed %d: %d tasks, %d acceptable, %d accepted, %d decided against the construction, %d differ from the DP, %d word/pair differences"
              % (seed, tasks, should, accepted, wrong, disagree, forms))
        assert n == tasks and tasks > 60000
        assert should > 20000 and accepted == should and wrong == 0
        assert disagree == 0
        assert forms == 0


@pytest.fixture(scope="module")
def bench_like(built):
    import oradrv
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    g, rs = bench_like_inputs()
    fa = os.path.join(tempfile.mkdtemp(prefix="arx_extc_"), "g.fa")
    g.write_fasta(fa)
    api.index_build(fa, fa, lib_path=SIM)
    ref = api.Reference(fa, lib_path=SIM)
    o = oradrv.Oracle(fa)
    ora = o.batch(rs.seqs, rs.lens, n_threads=8)
    yield ref, o, rs, ora
    ref.close()
    o.close()


def test_bench_like_reads_same_results_and_half_the_dps(bench_like, monkeypatch):
    ref, o, rs, ora = bench_like
    assert len(rs.lens) == 2 * 10010
    (off, c_off, _), (on, c_on, b) = run_both_ways(ref, rs.seqs, rs.lens, monkeypatch, keep=True)
    print("extension DPs %d -> %d, rounds %d -> %d" % (c_off["n_ext"], c_on["n_ext"], c_off["ext_rounds"], c_on["ext_rounds"]))
    assert_same_results(off, on)
    parity.check_core(b, o, rs.seqs, rs.lens)
    b.free()
    parity.check_final(on, ora)
    assert c_off["n_ext"] > 0 and 2 * c_on["n_ext"] <= c_off["n_ext"], (c_off, c_on)
    assert c_on["ext_rounds"] <= c_off["ext_rounds"], (c_off, c_on)


def test_golden_reads_same_results(built, monkeypatch):
    import oradrv
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    z = np.load(GOLD)
    prefix = workloads.unpack_index(z, tempfile.mkdtemp(prefix="arx_extc_"))
    ref = api.Reference(prefix, lib_path=SIM)
    o = oradrv.Oracle(prefix)
    seqs, lens = z["reads"][:400], z["lens"][:400]
    (off, c_off, _), (on, c_on, b) = run_both_ways(ref, seqs, lens, monkeypatch, keep=True)
    assert_same_results(off, on)
    parity.check_core(b, o, seqs, lens)
    b.free()
    parity.check_final(on, o.batch(seqs, lens))
    assert c_on["ext_rounds"] <= c_off["ext_rounds"], (c_off, c_on)
    ref.close()
    o.close()

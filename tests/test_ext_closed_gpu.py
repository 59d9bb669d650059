"""The extensions their diagonal decides (dev_sw.h ext_closed_form in KExtStep; ARX_EXT_CLOSED=0 switches it off) on the device: the
inputs and assertions of tests/test_ext_closed_hostsim.py, and a batch of 250-base reads with the switch on and off."""
import os
import tempfile

import numpy as np
import pytest

import parity
import workloads
from arachne_amd import api
from extclosed import assert_same_results, bench_like_inputs, run_both_ways

pytestmark = pytest.mark.gpu
GOLD = os.path.join(workloads.GOLDEN_DIR, "bwa_path_v1.npz")


def _open(g, name):
    fa = os.path.join(tempfile.mkdtemp(prefix="arx_gpu_extc_" + name), "g.fa")
    g.write_fasta(fa)
    api.index_build(fa, fa)
    ref = api.load_reference(fa, 0)
    assert ref.backend == "hip:gfx950"
    return fa, ref


def test_bench_like_reads_same_results_and_half_the_dps(built, monkeypatch):
    import oradrv
    g, rs = bench_like_inputs()
    fa, ref = _open(g, "bench")
    o = oradrv.Oracle(fa)
    (off, c_off, _), (on, c_on, b) = run_both_ways(ref, rs.seqs, rs.lens, monkeypatch, keep=True)
    print("extension DPs %d -> %d, rounds %d -> %d" % (c_off["n_ext"], c_on["n_ext"], c_off["ext_rounds"], c_on["ext_rounds"]))
    assert_same_results(off, on)
    parity.check_core(b, o, rs.seqs, rs.lens)
    b.free()
    parity.check_final(on, o.batch(rs.seqs, rs.lens, n_threads=8))
    assert c_off["n_ext"] > 0 and 2 * c_on["n_ext"] <= c_off["n_ext"], (c_off, c_on)
    assert c_on["ext_rounds"] <= c_off["ext_rounds"], (c_off, c_on)
    ref.close()
    o.close()


def test_golden_reads_same_results(built, monkeypatch):
    import oradrv
    z = np.load(GOLD)
    prefix = workloads.unpack_index(z, tempfile.mkdtemp(prefix="arx_gpu_extc_"))
    ref = api.load_reference(prefix, 0)
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


def test_long_reads_same_results(built, monkeypatch):
    """250-base reads (the widest extension class, a quarter of the reads corrupted): the switch changes nothing."""
    g, rs, seqs, lens = workloads.long_reads(250)
    assert len(lens) == 2 * 3 * 300
    fa, ref = _open(g, "long")
    (off, c_off, _), (on, c_on, _) = run_both_ways(ref, seqs, lens, monkeypatch)
    print("extension DPs %d -> %d, rounds %d -> %d" % (c_off["n_ext"], c_on["n_ext"], c_off["ext_rounds"], c_on["ext_rounds"]))
    assert_same_results(off, on)
    assert c_on["n_ext"] < c_off["n_ext"] and c_on["ext_rounds"] <= c_off["ext_rounds"], (c_off, c_on)
    ref.close()

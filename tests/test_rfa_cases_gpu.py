"""The planted placement cases (tests/rfacases.py; tests/test_rfa_cases_hostsim.py holds them to their claims) through libarachne_amd.so's
arx_selftest_rfa: RfaStage<HipRT>::run itself -- cand_count, cand_build, rfa, mapq_pair, mapq and the host MAPQ patch -- on one batch of 30
barcodes.  Here the chunked scan, the bitonic sort in LDS and in HBM (P = 8192), the strided cross-wave arg-max and the 256-lane class run on
what rfa_barcode really gives them; every candidate field, sum_move bit for bit and best_in_mol included, is compared with the restatement."""
import time

import numpy as np
import pytest

import rfacases
from arachne_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(built):
    c = rfacases.build()
    c["ora"] = rfacases.oracle(c)
    return c


def _run(case, what, **kw):
    t0 = time.time()
    dev = rfacases.run_device(case, api.LIB_PATH, **kw)
    print(f"\n[rfa cases gpu] {what}: {time.time() - t0:.2f} s, n_host_mapq {dev['n_host_mapq']} of {case['n_reads']} reads, small barcodes {int(dev['cls'].sum())}")
    return dev


def test_default(case):
    dev = _run(case, "default")
    rfacases.check_device(case, dev, np.zeros(len(case["barcodes"]), dtype=np.uint8))    # rfa_small off: no barcode ran small
    n_c = np.diff(dev["cand_off"][2 * case["bc_pair_off"]])
    p = np.array([1 << int(n - 1).bit_length() for n in n_c])
    assert (p > api.block_class(0)[1]).sum() >= 2, p                                                 # the sort in HBM ran
    assert (dev["cands"]["sum_move"] != 1.0).any() and ((dev["cands"]["best_in_mol"] == 1) & (dev["cands"]["active"] == 0)).any()


def test_rfa_small(case):
    dev = _run(case, "rfa_small", rfa_small=True)
    want = rfacases.small_class_rule(case)
    assert want.sum() >= 3
    rfacases.check_device(case, dev, want)                                              # exactly the barcodes the rule names ran small


def test_mapq_guard(case):
    """No value lies further than 0.5 from an integer: at a guard that wide RfaStage::run queues every read, capped ones included, for the host
    re-evaluation and the patch."""
    dev = _run(case, "guard 0.6", mapq_guard=0.6)
    rfacases.check_device(case, dev, np.zeros(len(case["barcodes"]), dtype=np.uint8))
    assert dev["n_host_mapq"] == case["n_reads"]


def test_second_call_in_one_process(case):
    a = _run(case, "first of two")
    b = _run(case, "second of two", rfa_small=True)
    c = _run(case, "third, default again")
    rfacases.check_device(case, b, rfacases.small_class_rule(case))
    rfacases.check_device(case, c, np.zeros(len(case["barcodes"]), dtype=np.uint8))
    for k in ("cand_off", "cands"):
        assert a[k].tobytes() == c[k].tobytes(), k                                      # nothing of a launch is left for the next
    for k in ("dna_len", "n_mol"):
        assert (a["barcodes"][k] == c["barcodes"][k]).all(), k

"""The rule that bins the backward sweeps' tasks by the length of their forward list (dev_fm.h seed_bwd_class), on the CPU.

The forward kernels' grant step (hip_fm_coop.h persistent_lanes) calls this function for every task it hands a pool slice to; the bins it fills
are what k_seed_bwd_g's 16 / 21 / 32 / 64-lane bodies work through.  The same header compiles for the host, so the function the kernel calls
is the one called here: either side of every edge, for the default middle bin and for ARX_SEED_BWD_MID=16, which leaves the 21-lane bin empty."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

HOSTSIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
LENGTHS = (0, 1, 16, 17, 21, 22, 32, 33, 64, 65)
# no bin for an empty list (a task whose pool slice overflowed has n = 0 too); <= 16 -> 0; <= mid -> 1; <= 32 -> 2; longer -> 3
WANT = {21: (-1, 0, 0, 1, 1, 2, 2, 3, 3, 3), 16: (-1, 0, 0, 2, 2, 2, 2, 3, 3, 3)}


@pytest.fixture(scope="module")
def rule():
    so = os.path.join(tempfile.mkdtemp(prefix="arx_seed_bins_unit_"), "libarx_seed_bins.so")   # dev_fm.h for the host, on its own
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-o", so, os.path.join(HOSTSIM, "seed_bins.cpp")])
    lib = C.CDLL(so)
    lib.arx_test_seed_bwd_class.restype = None
    lib.arx_test_seed_bwd_class.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]

    def classes(lens, mid):
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        out = np.full(len(lens), -9, dtype=np.int32)
        lib.arx_test_seed_bwd_class(len(lens), lens.ctypes.data, mid, out.ctypes.data)
        return out
    return classes


@pytest.mark.parametrize("mid", [21, 16])
def test_class_either_side_of_every_edge(rule, mid):
    got = rule(LENGTHS, mid)
    assert tuple(int(c) for c in got) == WANT[mid], (mid, got)


@pytest.mark.parametrize("mid", [21, 16])
def test_class_is_the_smallest_group_that_holds_the_list(rule, mid):
    """Every length up to two wavefronts: the class's group (16, mid, 32 lanes) holds the list and the class below does not; the last class
    takes what no group holds in one row (k_seed_bwd_g hands lists of more than 64 entries on to k_seed_bwd_wave)."""
    lens = np.arange(0, 130)
    got = rule(lens, mid)
    cap = (16, mid, 32)
    for n, c in zip(lens, got):
        if n == 0:
            assert c == -1
            continue
        want = next((k for k in range(3) if n <= cap[k]), 3)
        assert c == want, (n, c, want)
    if mid == 16:
        assert not (got == 1).any()

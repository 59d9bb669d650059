"""The library's request for hardware queues when it is loaded, and the default of the side streams that follows it (switches.h
sw_request_hw_queues, arx_side_streams_default).

The HIP runtime reads GPU_MAX_HW_QUEUES once, when it is initialised.  Loaded into a process that has not opened the GPU, the library raises
the variable to ARX_HW_QUEUES (8) and batch handles use their side streams by default; loaded into a process that has (the HSA runtime then
holds /dev/kfd open) with fewer queues than that, it leaves the variable alone and handles run on one stream unless ARX_AUX_STREAM=1 forces
them -- on shared queues the side streams cost 10 % of the throughput (profiles/side_stream/README.md).  What matters is the order of two
events in a process's life, so every case is a fresh child process; the cases that open the GPU first need one (-m gpu)."""
import os
import subprocess
import sys

import pytest

from arachne_amd import api

CHILD = r"""
import ctypes, sys
libc = ctypes.CDLL(None)
libc.getenv.restype = ctypes.c_char_p
if sys.argv[2] == "gpu_first":
    hip = ctypes.CDLL("libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
    n = ctypes.c_int(0)
    assert hip.hipInit(0) == 0 and hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value >= 1
lib = ctypes.CDLL(sys.argv[1])
lib.arx_side_streams_default.restype = ctypes.c_int32
v = libc.getenv(b"GPU_MAX_HW_QUEUES")
print("RESULT", lib.arx_side_streams_default(), v.decode() if v is not None else "unset")
"""


def child(order, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "ARX_HW_QUEUES", "ARX_AUX_STREAM")}
    e.update({k: str(v) for k, v in env.items()})
    e["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + e.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([sys.executable, "-c", CHILD, api.LIB_PATH, order], env=e, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()
    return int(line[1]), line[2]


@pytest.mark.parametrize("env, want", [
    ({}, (1, "8")),                                                  # unset: raised to 8
    ({"GPU_MAX_HW_QUEUES": 4}, (1, "8")),                            # lower: raised
    ({"GPU_MAX_HW_QUEUES": 16}, (1, "16")),                          # enough: left alone
    ({"GPU_MAX_HW_QUEUES": 4, "ARX_HW_QUEUES": 12}, (1, "12")),
    ({"GPU_MAX_HW_QUEUES": 4, "ARX_HW_QUEUES": 99}, (1, "32")),      # never above 32
    ({"GPU_MAX_HW_QUEUES": 4, "ARX_HW_QUEUES": 0}, (0, "4")),        # no request: the side streams would share queues
    ({"GPU_MAX_HW_QUEUES": 4, "ARX_AUX_STREAM": 0}, (0, "4")),       # the opt-out at load time: no request
    ({"ARX_AUX_STREAM": 0}, (0, "unset")),
], ids=lambda x: ",".join(f"{k}={v}" for k, v in x.items()) or "unset" if isinstance(x, dict) else None)
def test_library_loaded_first(built, env, want):
    assert child("library_first", **env) == want


@pytest.mark.gpu
@pytest.mark.parametrize("env, want", [
    ({"GPU_MAX_HW_QUEUES": 4}, (0, "4")),                            # too late: the variable stays, the side streams are off by default
    ({}, (0, "unset")),                                              # the runtime's own 4
    ({"GPU_MAX_HW_QUEUES": 8}, (1, "8")),                            # the launcher set it: on
    ({"GPU_MAX_HW_QUEUES": 16}, (1, "16")),
], ids=lambda x: ",".join(f"{k}={v}" for k, v in x.items()) or "unset" if isinstance(x, dict) else None)
def test_gpu_opened_first(built, env, want):
    assert child("gpu_first", **env) == want

"""CPU test of the device BGZF compressor's logic (arachne_amd/csrc/dev_bgzf.h): tests/bgzfsim/bgzf_sim.cpp compiles the very functions the
kernel runs, with the lanes of a workgroup in a loop, under -fsanitize=address,undefined, and is run as a plain process.  Every block it
writes is inflated and checksummed by Python's zlib (bgzfcases.py); the code builder is held to its contract on count vectors."""
import os
import subprocess
from fractions import Fraction

import pytest

import bgzfcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bgzfsim") / "bgzf_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "bgzfsim", "bgzf_sim.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def cases():
    return bgzfcases.edge_inputs()


def _deflate(sim, tmp, data, rev=False):
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bgzf")
    with open(src, "wb") as f:
        f.write(data)
    r = subprocess.run([sim, "deflate", src, dst] + (["rev"] if rev else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    b, s, f, d = (int(x) for x in r.stdout.split())
    with open(dst, "rb") as fh:
        return fh.read(), dict(blocks=b, stored=s, fixed=f, dynamic=d)


def test_edge_inputs_inflate_to_the_input(sim, cases, tmp_path):
    for name, data in cases.items():
        raw, forms = _deflate(sim, str(tmp_path), data)
        bgzfcases.check_case(name, data, raw, forms)
    # the forms are all taken: tiny inputs fixed, text dynamic, random bytes stored; and distance 32769 is never used (zlib would refuse it)
    assert _deflate(sim, str(tmp_path), cases["a_text_3"])[1]["fixed"] == 1
    assert _deflate(sim, str(tmp_path), cases["a_text_65280"])[1]["dynamic"] == 1
    raw_d, _ = _deflate(sim, str(tmp_path), cases["d_distance_32768"])
    raw_e, _ = _deflate(sim, str(tmp_path), cases["e_distance_32769"])
    assert len(raw_d) < len(cases["d_distance_32768"]) and len(raw_e) >= 65280


def test_bytes_do_not_depend_on_the_order_of_the_lanes(sim, cases, tmp_path):
    for name in ("a_text_130561", "c_record300", "h_fibonacci", "g_two_values"):
        assert _deflate(sim, str(tmp_path), cases[name])[0] == _deflate(sim, str(tmp_path), cases[name], rev=True)[0], name


def test_it_compresses_a_bam_like_stream(sim, tmp_path):
    import zlib
    data = bgzfcases.bam_like_stream(1000)
    raw, forms = _deflate(sim, str(tmp_path), data)
    bgzfcases.check_stream(raw, data)
    assert forms["stored"] == 0
    assert len(raw) < bgzfcases.zlib_size(data, zlib.Z_FIXED) and len(raw) < bgzfcases.zlib_size(data, zlib.Z_HUFFMAN_ONLY)


def _code(sim, limit, freq):
    r = subprocess.run([sim, "code", str(limit), str(len(freq))] + [str(f) for f in freq], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lens = [int(x) for x in r.stdout.split()]
    assert len(lens) == len(freq)
    return lens


def _clipped_fibonacci(k, total):
    out, left = [], total
    for f in bgzfcases.fibonacci(k):
        out.append(min(f, left))
        left -= out[-1]
    return out


@pytest.mark.parametrize("limit,n_sym", [(15, 286), (15, 30), (7, 19)])
def test_code_builder(sim, limit, n_sym):
    k = min(30, n_sym)
    fib = _clipped_fibonacci(k, 65280) + [0] * (n_sym - k)
    assert sum(fib) == 65280 or k < 24
    vectors = {"fibonacci": fib, "fibonacci_reversed": fib[::-1], "single": [0] * (n_sym - 1) + [9], "two": [5] + [0] * (n_sym - 2) + [1],
               "all_equal": [7] * n_sym, "ramp": list(range(n_sym))}
    for name, freq in vectors.items():
        lens = _code(sim, limit, freq)
        used = [l for l, f in zip(lens, freq) if f]
        assert all(l == 0 for l, f in zip(lens, freq) if not f), name
        assert all(1 <= l <= limit for l in used), (name, lens)
        if len(used) >= 2:
            assert sum(Fraction(1, 2 ** l) for l in used) == 1, (name, lens)
        else:
            assert used == [1], name
        by_count = sorted(zip(freq, lens))
        assert all(a[1] >= b[1] for a, b in zip(by_count, by_count[1:]) if a[0] and a[0] < b[0]), name  # a rarer symbol never has the shorter code
    # where the limit does not bind, the code is a Huffman code: its cost is the optimum (checked against a heap-built one)
    import heapq
    freq = vectors["ramp"]
    heap = [f for f in freq if f]
    heapq.heapify(heap)
    best = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        best += a + b
        heapq.heappush(heap, a + b)
    lens = _code(sim, limit, freq)
    if max(lens) < limit:
        assert sum(f * l for f, l in zip(freq, lens)) == best

"""CPU test of the full records phase's device logic (arachne_amd/csrc/dev_records_full.h): tests/recsim/rec_full_sim.cpp compiles the very
functors arx_batch_records_full launches, runs them as loops, ascending and descending, over arrays of exactly the sizes they may touch,
under -fsanitize=address,undefined as a plain process, and compares both streams, the buckets and both offset tables byte for byte with the
host path (RecBuf::build in its full mode + BamSink::encode, and the stable order of that by bucket) on random cases; the program itself
refuses a run whose cases did not hold what its header lists.  Both sides take the rules from csrc/bam_rules.h, so that comparison cannot see
a mistake inside them: the program also prints a digest of the host path's stream and buckets, pinned in
tests/golden/records_full_stream_v1.json to what it printed before the rules were shared.  Its second mode holds the two decimal formatters
to snprintf."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("recfullsim") / "rec_full_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "recsim", "rec_full_sim.cpp"), "-o", exe, "-lz", "-pthread"])
    return exe


@pytest.mark.parametrize("order", [[], ["rev"]])
def test_functors_write_the_host_paths_streams(sim, order):
    with open(os.path.join(ROOT, "tests", "golden", "records_full_stream_v1.json")) as f:
        pin = json.load(f)
    r = subprocess.run([sim, str(pin["seed"]), str(pin["cases"])] + order, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.split() == [str(pin["cases"]), pin["digest"]]


def _ties():
    """(ties, those whose value is no double) among n = 128, 256, ... 32768 (a tie needs 128 | n) and s <= 4 n: 2 s 10^6 / n = 2 k + 1 means
    s / n = (2 k + 1) / (2^7 5^6), which is a binary fraction only when 5^6 divides 2 k + 1"""
    ties = odd_ones = 0
    for n in range(128, 32769, 128):
        for s in range(4 * n + 1):
            a = 2000000 * s
            if a % n == 0 and (a // n) & 1:
                ties += 1
                odd_ones += (a // n) % 15625 != 0
    return ties, odd_ones


def test_decimal_text_is_snprintfs(sim):
    r = subprocess.run([sim, "text"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    n_dm, n_tie, n_int = map(int, r.stdout.split())
    ties, not_doubles = _ties()
    assert not_doubles >= 100
    assert n_tie == ties
    assert n_dm >= sum(4 * n + 1 for n in range(1, 513)) + 200000 and n_int >= 64

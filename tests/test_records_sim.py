"""CPU test of the records phase's device logic (arachne_amd/csrc/dev_records.h): tests/recsim/rec_sim.cpp compiles the very functors
arx_batch_records launches, runs them as loops over arrays of exactly the sizes the stage driver allocates, under
-fsanitize=address,undefined as a plain process, and compares the stream byte for byte with the host path (RecBuf::build + BamSink::encode)
on random cases: reads of 0..255 bases, names of 1 and 254 bytes, empty read groups, barcodes and sets, placeholders, two active candidates,
long CIGAR runs, positions up to 2^30.  Both sides take the rules of a record's fields from csrc/bam_rules.h, so that comparison cannot see a
mistake inside them: the program also prints a digest of the host path's stream, pinned in tests/golden/records_stream_v1.json to what it
printed before the rules were shared."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("recsim") / "rec_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "recsim", "rec_sim.cpp"), "-o", exe, "-lz", "-pthread"])
    return exe


@pytest.mark.parametrize("order", [[], ["rev"]])
def test_functors_write_the_host_paths_stream(sim, order):
    r = subprocess.run([sim, "3", "400"] + order, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    with open(os.path.join(ROOT, "tests", "golden", "records_stream_v1.json")) as f:
        pin = json.load(f)
    assert (pin["seed"], pin["cases"]) == (3, 400)
    assert r.stdout.split() == ["400", pin["digest"]["rev" if order else "ascending"]]

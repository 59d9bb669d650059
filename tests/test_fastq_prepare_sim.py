"""CPU test of the fused standardize-and-sort's device logic (arachne_amd/csrc/dev_fqprep.h over dev_fqstd.h, dev_fqsort.h and dev_fqmerge.h):
tests/fqprepsim/fastq_prepare_sim.cpp compiles the very functors and drivers the kernels run -- the fields and the key in two pieces per record
of the table, the order through the key accessor, the composing gather, the runs of raw text with their keys kept whole -- under
-fsanitize=address,undefined and is run as a plain process.  Every small case of fqprepcases.py runs with both texts in memory and at three run
sizes, each at three windows, two slab sizes and with the items ascending and descending, every buffer an allocation of exactly its size (the
program itself holds those twelve runs to one another); output bytes, record offsets and counts of all run sizes are compared with
fqprepcases' expectation, the two restatements composed, which knows neither of runs nor of the key's pieces."""
import os
import subprocess

import pytest

import fqprepcases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS_E_TOO_LARGE, FS_E_RUN, SIM_UNKNOWN = 1, 3, 9
NAMES = ("status", "format", "decided", "n", "skipped", "runs", "distinct", "longest", "with_bc", "valid", "sorted_runs")


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fqprepsim") / "fastq_prepare_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "fqprepsim", "fastq_prepare_sim.cpp"), "-o", exe])
    return exe


def _run(sim, tmp, name, c, run_bytes, windows=None):
    """c: a fqprepcases.Case -> (return code, stderr, {run_bytes: dict(NAMES ..., off1, off2, out1, out2)})"""
    p1, p2 = os.path.join(tmp, name + ".in1"), os.path.join(tmp, name + ".in2")
    for p, t in ((p1, c.t1), (p2, c.t2)):
        with open(p, "wb") as f:
            f.write(t)
    manifest = os.path.join(tmp, "manifest.txt")
    with open(manifest, "w") as f:
        f.writelines("%s %s %s %d %d %s\n" % (name, p1, p2, c.format, rb, ",".join(str(w) for w in (windows or c.windows))) for rb in run_bytes)
    r = subprocess.run([sim, manifest, tmp], capture_output=True, text=True)
    got, cur = {}, None
    for l in r.stdout.splitlines():
        w = l.split()
        if w[0] == "case":
            cur = got[int(w[2])] = dict(zip(NAMES, (int(x) for x in w[3:])))
        else:
            cur[w[0]] = [int(x) for x in w[1:]]
    for rb, g in got.items():
        if g["status"] == 0:
            g["out1"], g["out2"] = (open(os.path.join(tmp, "%s.%d%s" % (name, rb, e)), "rb").read() for e in (".r1", ".r2"))
    return r.returncode, r.stderr, got


def _hold(name, c, g):
    assert g["status"] == 0, name
    assert (g["format"], g["decided"]) == (c.found, c.decided), name
    assert (g["n"], g["skipped"], g["runs"], g["distinct"], g["longest"]) == (c.n, c.skipped, c.runs, c.distinct, c.longest), name
    assert (g["with_bc"], g["valid"]) == (c.with_bc, c.valid), name
    assert g["out1"] == c.out1 and g["out2"] == c.out2, name
    assert g["off1"] == c.off1.tolist() and g["off2"] == c.off2.tolist(), name


def test_the_cases_are_what_they_claim():
    pc.check_cases()


@pytest.mark.parametrize("name", pc.GOOD)
def test_cases_in_core_and_in_runs(sim, tmp_path, name):
    c = pc.cases()[name]
    sizes = (0,) + tuple(c.run_bytes)
    rc, err, got = _run(sim, str(tmp_path), name, c, sizes)
    assert rc == 0 and sorted(got) == sorted(sizes), (rc, err[-4000:])
    for rb in sizes:
        _hold(name, c, got[rb])
        if rb and "runs" in c.claims:
            assert got[rb]["sorted_runs"] >= len(c.t1) // rb, (name, rb)


@pytest.mark.parametrize("name", pc.UNKNOWN_CASES)
def test_no_format_is_found(sim, tmp_path, name):
    c = pc.cases()[name]
    rc, err, got = _run(sim, str(tmp_path), name, c, (0, 4096))
    assert rc == 0, (rc, err[-2000:])
    for rb in (0, 4096):
        assert got[rb]["status"] == SIM_UNKNOWN and (got[rb]["format"], got[rb]["decided"]) == (pc.UNKNOWN, -1) and "off1" not in got[rb], (name, got)


def test_a_record_longer_than_the_window_or_the_run(sim, tmp_path):
    c = pc.cases()["std_bc300"]
    assert max(len(r[0]) for r in c.std.recs) > 256
    rc, err, got = _run(sim, str(tmp_path), "long", c, (0, 4096), windows=(128, 256, 256))
    assert rc == 0 and got[0]["status"] == got[4096]["status"] == FS_E_TOO_LARGE and "off1" not in got[0], (rc, err[-2000:], got)
    rc, err, got = _run(sim, str(tmp_path), "long", c, (256,))
    assert rc == 0 and got[256]["status"] in (FS_E_TOO_LARGE, FS_E_RUN) and "off1" not in got[256], (rc, err[-2000:], got)


def test_a_few_thousand_records(sim, tmp_path):
    c = pc.cases()["std_many"]
    rc, err, got = _run(sim, str(tmp_path), "many", c, (0, 65536), windows=(4096, 65536, 65536))
    assert rc == 0, (rc, err[-4000:])
    _hold("many", c, got[0])
    _hold("many", c, got[65536])
    assert got[65536]["sorted_runs"] >= 4

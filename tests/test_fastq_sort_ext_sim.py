"""CPU test of the external FASTQ sort's device logic (arachne_amd/csrc/dev_fqmerge.h over dev_fqsort.h): tests/fqextsim/fastq_sort_ext_sim.cpp
compiles the very functors and drivers the kernels run -- runs with open ends and carries, the kept keys, the rank queries, the merge gather
from staged ranges -- under -fsanitize=address,undefined and is run as a plain process.  Every small case of fqsortcases.py and every case of
fqextcases.py runs at three run sizes, the smallest window, two slab sizes and with the items ascending and descending, every buffer an
allocation of exactly its size; output bytes, record offsets and counts are compared with fqsortcases' restatement, which does not know of
runs, and the number of sorted runs with the least the case's bytes require."""
import os
import subprocess

import pytest

import fqextcases as xc
import fqsortcases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fqextsim") / "fastq_sort_ext_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "fqextsim", "fastq_sort_ext_sim.cpp"), "-o", exe])
    return exe


def _run(sim, tmp, name, c, run_bytes, mode="all"):
    """c: a fqsortcases.Case -> (return code, stderr, {run_bytes: dict(status, n, skipped, runs, distinct, longest, sorted_runs, file_bytes, off1, off2, out1, out2)})"""
    p1, p2 = os.path.join(tmp, name + ".in1"), os.path.join(tmp, name + ".in2")
    for p, t in ((p1, c.t1), (p2, c.t2)):
        with open(p, "wb") as f:
            f.write(t)
    manifest = os.path.join(tmp, "manifest.txt")
    with open(manifest, "w") as f:
        f.writelines("%s %s %s %d %s\n" % (name, p1, p2, rb, mode) for rb in run_bytes)
    r = subprocess.run([sim, manifest, tmp], capture_output=True, text=True)
    got, cur = {}, None
    for l in r.stdout.splitlines():
        w = l.split()
        if w[0] == "case":
            cur = got[int(w[2])] = dict(zip(("status", "n", "skipped", "runs", "distinct", "longest", "sorted_runs", "file_bytes"), (int(x) for x in w[3:])))
        else:
            cur[w[0]] = [int(x) for x in w[1:]]
    for rb, g in got.items():
        if g["status"] == 0:
            g["out1"], g["out2"] = (open(os.path.join(tmp, "%s.%d%s" % (name, rb, e)), "rb").read() for e in (".r1", ".r2"))
    return r.returncode, r.stderr, got


def _hold(name, c, g):
    assert g["status"] == 0, name
    assert (g["n"], g["skipped"], g["runs"], g["distinct"], g["longest"]) == (c.n, c.skipped, c.runs, c.distinct, c.longest), name
    assert g["out1"] == c.out1 and g["out2"] == c.out2, name
    assert g["off1"] == c.off1.tolist() and g["off2"] == c.off2.tolist(), name
    assert g["file_bytes"] == len(c.out1) + len(c.out2), name            # the run files hold every record once


def test_the_cases_are_what_they_claim():
    fc.check_cases()
    xc.check_cases()


@pytest.mark.parametrize("name", fc.SMALL)
def test_small_cases_in_runs(sim, tmp_path, name):
    c = fc.cases()[name]
    rc, err, got = _run(sim, str(tmp_path), name, c, xc.RUN_BYTES)
    assert rc == 0 and sorted(got) == sorted(xc.RUN_BYTES), (rc, err[-4000:])
    for rb in xc.RUN_BYTES:
        _hold(name, c, got[rb])
        assert got[rb]["sorted_runs"] >= xc.least_runs(c, rb), (name, rb)


@pytest.mark.parametrize("name", xc.GOOD)
def test_run_borders(sim, tmp_path, name):
    x = xc.cases()[name]
    rc, err, got = _run(sim, str(tmp_path), name, x.case, xc.RUN_BYTES)
    assert rc == 0 and sorted(got) == sorted(xc.RUN_BYTES), (rc, err[-4000:])
    for rb in xc.RUN_BYTES:
        _hold(name, x.case, got[rb])
        assert got[rb]["sorted_runs"] >= xc.least_runs(x.case, rb), (name, rb)
    assert got[x.run_bytes]["sorted_runs"] >= x.min_runs
    if x.exact_runs is not None:
        assert got[x.run_bytes]["sorted_runs"] == x.exact_runs


@pytest.mark.parametrize("name", xc.REFUSED)
def test_refused(sim, tmp_path, name):
    x = xc.cases()[name]
    rc, err, got = _run(sim, str(tmp_path), name, x.case, (x.run_bytes,))
    assert rc == 0 and got[x.run_bytes]["status"] == x.status and "off1" not in got[x.run_bytes], (rc, err[-2000:], got)


def test_the_cap_itself_is_allowed(sim, tmp_path):
    t1, t2 = xc._over_cap()
    c = fc.Case(t1[:-4 * 32], t2[:-len(b"".join(r[1] for r in xc.cases()["over_cap"].case.recs[-4:]))])
    assert xc.least_runs(c, 128) == xc.MAX_RUNS
    rc, err, got = _run(sim, str(tmp_path), "cap", c, (128,), mode="once")
    assert rc == 0, (rc, err[-2000:])
    _hold("cap", c, got[128])
    assert got[128]["sorted_runs"] == xc.MAX_RUNS


def test_many_records_in_sixteen_runs(sim, tmp_path):
    c = fc.cases()["many"]
    rb = 150000
    assert xc.least_runs(c, rb) >= 16
    rc, err, got = _run(sim, str(tmp_path), "many", c, (rb,), mode="once")
    assert rc == 0, (rc, err[-4000:])
    _hold("many", c, got[rb])
    assert got[rb]["sorted_runs"] >= 16

"""CPU test of the FASTQ sort's device logic (arachne_amd/csrc/dev_fqsort.h): tests/fqsortsim/fastq_sort_sim.cpp compiles the very functions
the kernels run -- the feeder's functors of dev_fastq.h among them --, with the items of a launch in a loop, under
-fsanitize=address,undefined, and is run as a plain process.  Every case of fqsortcases.py runs at three window sizes, two slab sizes and
with the items in ascending and in descending order, every buffer an allocation of exactly its size (the program holds the twelve runs to
one another and to what the case's line claims); output bytes, record offsets and counts are compared with fqsortcases' restatement."""
import os
import subprocess

import pytest

import fqsortcases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fqsortsim") / "fastq_sort_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "fqsortsim", "fastq_sort_sim.cpp"), "-o", exe])
    return exe


def _run(sim, tmp, cases):
    """cases: {name: Case} -> (return code, stderr, {name: dict(status, n, skipped, runs, distinct, longest, off1, off2, out1, out2)})"""
    lines = []
    for name, c in cases.items():
        p1, p2 = os.path.join(tmp, name + ".in1"), os.path.join(tmp, name + ".in2")
        for p, t in ((p1, c.t1), (p2, c.t2)):
            with open(p, "wb") as f:
                f.write(t)
        lines.append("%s %s %s %s\n" % (name, p1, p2, ",".join(c.claims) or "-"))
    manifest = os.path.join(tmp, "manifest.txt")
    with open(manifest, "w") as f:
        f.writelines(lines)
    r = subprocess.run([sim, manifest, tmp], capture_output=True, text=True)
    got, cur = {}, None
    for l in r.stdout.splitlines():
        w = l.split()
        if w[0] == "case":
            cur = got[w[1]] = dict(zip(("status", "n", "skipped", "runs", "distinct", "longest"), (int(x) for x in w[2:])))
        else:
            cur[w[0]] = [int(x) for x in w[1:]]
    for name, g in got.items():
        if g["status"] == 0:
            g["out1"], g["out2"] = (open(os.path.join(tmp, name + e), "rb").read() for e in (".r1", ".r2"))
    return r.returncode, r.stderr, got


def _hold(name, c, g):
    assert g["status"] == 0, name
    assert (g["n"], g["skipped"], g["runs"], g["distinct"], g["longest"]) == (c.n, c.skipped, c.runs, c.distinct, c.longest), name
    assert g["out1"] == c.out1 and g["out2"] == c.out2, name
    assert g["off1"] == c.off1.tolist() and g["off2"] == c.off2.tolist(), name


def test_the_cases_are_what_they_claim():
    fc.check_cases()


@pytest.mark.parametrize("name", fc.SMALL)
def test_sort(sim, tmp_path, name):
    c = fc.cases()[name]
    rc, err, got = _run(sim, str(tmp_path), {name: c})
    assert rc == 0, (rc, err[-4000:])
    _hold(name, c, got[name])


def test_many_records(sim, tmp_path):
    c = fc.cases()["many"]
    rc, err, got = _run(sim, str(tmp_path), {"many": c})
    assert rc == 0, (rc, err[-4000:])
    _hold("many", c, got["many"])


def test_a_claim_that_is_not_met_is_reported(sim, tmp_path):
    c = fc.cases()["one"]
    for claim in ("windows", "blocks", "slabs", "chunks", "skipped", "align", "large"):
        rc, err, got = _run(sim, str(tmp_path), {"one": fc.Case(c.t1, c.t2, claims=(claim,))})
        assert rc == 4 and claim in err, (claim, rc, err[-1000:])


def test_a_record_longer_than_every_window_is_refused(sim, tmp_path):
    t1, t2 = fc.pair(b"long", b"A-1", 5, 5)
    c = fc.Case(t1.replace(b"@long", b"@" + b"n" * 5000), t2)
    rc, err, got = _run(sim, str(tmp_path), {"long": c})
    assert rc == 0 and got["long"]["status"] == 1 and "off1" not in got["long"], (rc, err[-1000:])     # FS_E_TOO_LARGE at all three sizes


def test_window_sizes_that_disagree_are_reported(sim, tmp_path):
    t1, t2 = fc.pair(b"long", b"A-1", 5, 5)
    c = fc.Case(t1.replace(b"@long", b"@" + b"n" * 200), t2)           # the smallest window refuses it, the larger ones do not
    rc, err, got = _run(sim, str(tmp_path), {"long": c})
    assert rc == 3 and "disagrees" in err

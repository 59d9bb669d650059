"""CPU test of the header standardization's device logic (arachne_amd/csrc/dev_fqstd.h): tests/fqstdsim/fastq_std_sim.cpp compiles the very
functions the kernels run -- the feeder's line and record functors of dev_fastq.h among them --, with the items of a launch in a loop, under
-fsanitize=address,undefined, and is run as a plain process.  Every case of fqstdcases.py runs at three window sizes, two slab sizes and with
the items in ascending and in descending order, every buffer an allocation of exactly its size (the program holds the twelve runs to one
another and to what the case's line claims); output bytes, record offsets, format, deciding record and counts are compared with fqstdcases'
restatement."""
import os
import subprocess

import pytest

import fqstdcases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fqstdsim") / "fastq_std_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "fqstdsim", "fastq_std_sim.cpp"), "-o", exe])
    return exe


def _run(sim, tmp, cases):
    """cases: {name: Case} -> (return code, stderr, {name: dict(status, format, decided, written, n, skipped, with_bc, valid, longest, off1, off2, out1, out2)})"""
    lines = []
    for name, c in cases.items():
        p1, p2 = os.path.join(tmp, name + ".in1"), os.path.join(tmp, name + ".in2")
        for p, t in ((p1, c.t1), (p2, c.t2)):
            with open(p, "wb") as f:
                f.write(t)
        lines.append("%s %s %s %d %s\n" % (name, p1, p2, c.format, ",".join(c.claims) or "-"))
    manifest = os.path.join(tmp, "manifest.txt")
    with open(manifest, "w") as f:
        f.writelines(lines)
    r = subprocess.run([sim, manifest, tmp], capture_output=True, text=True)
    got, cur = {}, None
    for l in r.stdout.splitlines():
        w = l.split()
        if w[0] == "case":
            cur = got[w[1]] = dict(zip(("status", "format", "decided", "written", "n", "skipped", "with_bc", "valid", "longest"), (int(x) for x in w[2:])))
        else:
            cur[w[0]] = [int(x) for x in w[1:]]
    for name, g in got.items():
        if g["status"] == 0 and g["written"]:
            g["out1"], g["out2"] = (open(os.path.join(tmp, name + e), "rb").read() for e in (".r1", ".r2"))
    return r.returncode, r.stderr, got


def _hold(name, c, g):
    assert g["status"] == 0, name
    if c.format == sc.AUTO:
        assert (g["format"], g["decided"]) == (c.found, c.decided), name
    else:
        assert (g["format"], g["decided"]) == (c.format, -1), name
    assert g["written"] == (c.used is not None), name
    if c.used is None:
        return
    assert (g["n"], g["skipped"], g["with_bc"], g["valid"], g["longest"]) == (c.n, c.skipped, c.with_bc, c.valid, c.longest), name
    assert g["out1"] == c.out1 and g["out2"] == c.out2, name
    assert g["off1"] == c.off1.tolist() and g["off2"] == c.off2.tolist(), name


def test_the_cases_are_what_they_claim():
    sc.check_cases()


def test_small_cases(sim, tmp_path):
    cs = {n: sc.cases()[n] for n in sc.SMALL}
    rc, err, got = _run(sim, str(tmp_path), cs)
    assert rc == 0, (rc, err[-4000:])
    assert set(got) == set(cs)
    for name, c in cs.items():
        _hold(name, c, got[name])


def test_many_records(sim, tmp_path):
    c = sc.cases()["many"]
    rc, err, got = _run(sim, str(tmp_path), {"many": c})
    assert rc == 0, (rc, err[-4000:])
    _hold("many", c, got["many"])


def test_a_claim_that_is_not_met_is_reported(sim, tmp_path):
    c = sc.cases()["det_stlfr_eol"]
    for claim in ("windows", "slabs", "skipped", "align"):
        rc, err, got = _run(sim, str(tmp_path), {"one": sc.Case(c.t1, c.t2, claims=(claim,))})
        assert rc == 4 and claim in err, (claim, rc, err[-1000:])


def test_a_record_longer_than_every_window_is_refused(sim, tmp_path):
    t1, t2 = sc.rec(b"long#1_2_3", 5, 5)
    c = sc.Case(t1.replace(b"@long", b"@" + b"n" * 5000), t2)
    rc, err, got = _run(sim, str(tmp_path), {"long": c})
    assert rc == 0 and got["long"]["status"] == 1 and "off1" not in got["long"], (rc, err[-1000:])     # FS_E_TOO_LARGE at all three sizes
    c = sc.Case(c.t1, c.t2, fmt=sc.STLFR)                                                              # in the conversion as in the detection
    rc, err, got = _run(sim, str(tmp_path), {"long": c})
    assert rc == 0 and got["long"]["status"] == 1 and "off1" not in got["long"], (rc, err[-1000:])


def test_window_sizes_that_disagree_are_reported(sim, tmp_path):
    t1, t2 = sc.rec(b"long#1_2_3", 5, 5)
    c = sc.Case(t1.replace(b"@long", b"@" + b"n" * 200), t2)           # the smallest window refuses it, the larger ones do not
    rc, err, got = _run(sim, str(tmp_path), {"long": c})
    assert rc == 3 and "disagrees" in err

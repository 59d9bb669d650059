"""CPU test of the FASTA pack's device logic (arachne_amd/csrc/dev_fapack.h, behind arx_index_build_ex): tests/fapacksim/fasta_pack_sim.cpp
compiles the very functions the kernels run, with the items of a launch in a loop, under -fsanitize=address,undefined, and is run as a plain
process.  Every case of fapackcases.py runs at three window sizes with the items in ascending and in descending order, every buffer an
allocation of exactly its size; the program holds the six runs to one another, to the files of fapackcases' restatement and to build_index
(index_build.h) on the same file, and this test compares the rows it prints with the restatement's.  Where the reference's own library is
built (oracle/_ref), the restatement's files of the well-formed cases are compared with the reference's bwa_idx_build."""
import os
import subprocess

import pytest

import fapackcases as fc
import refdrv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fapacksim") / "fasta_pack_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "fapacksim", "fasta_pack_sim.cpp"), "-o", exe])
    return exe


def _run(sim, tmp, cases, claims=None, want=None):
    """cases: {name: Case}; claims: {name: "a,b"}; want: {name: Case} whose files stand for the restatement's (the cases' own by default)
    -> (return code, stderr, {name: dict(status, l_pac, n_contigs, n_holes, n_amb, cnt, contigs, holes, pac, ann, amb)})"""
    lines = []
    for name, c in cases.items():
        p = os.path.join(tmp, name + ".fa")
        w = (want or cases)[name]
        for path, data in ((p, c.text), (p + ".want.pac", w.pac_file()), (p + ".want.ann", w.ann_file()), (p + ".want.amb", w.amb_file())):
            with open(path, "wb") as f:
                f.write(data)
        lines.append("%s %s %d %s\n" % (name, p, w.status, (claims or {}).get(name, "-")))
    manifest = os.path.join(tmp, "manifest.txt")
    with open(manifest, "w") as f:
        f.writelines(lines)
    r = subprocess.run([sim, manifest, tmp], capture_output=True, text=True)
    got, cur = {}, None
    for l in r.stdout.splitlines():
        w = l.split()
        if w[0] == "case":
            v = [int(x) for x in w[2:]]
            cur = got[w[1]] = dict(status=v[0], l_pac=v[1], n_contigs=v[2], n_holes=v[3], n_amb=v[4], cnt=v[5:9], contigs=[], holes=[])
        else:
            cur[w[0] + "s"].append(tuple(int(x) for x in w[1:]))
    for name, g in got.items():
        if g["status"] == 0:
            for e in ("pac", "ann", "amb"):
                g[e] = open(os.path.join(tmp, name + "." + e), "rb").read()
    return r.returncode, r.stderr, got


def _hold(name, c, g):
    assert g["status"] == c.status, name
    if c.status != fc.OK:
        return
    assert (g["l_pac"], g["n_contigs"], g["n_holes"], g["n_amb"], g["cnt"]) == (c.l_pac, len(c.contigs), len(c.holes), c.n_amb, c.cnt), name
    assert g["contigs"] == c.contigs and g["holes"] == c.holes, name
    assert g["pac"] == c.pac_file() and g["ann"] == c.ann_file() and g["amb"] == c.amb_file(), name


CLAIMS = {"hdr300": "windows,header", "single_line": "windows,codes", "many": "windows,header,codes", "cut_behind_gt": "windows,header", "cut_pac_1": "windows,codes"}


def test_the_cases_are_what_they_claim():
    fc.check_cases()


def test_small_cases(sim, tmp_path):
    cs = {n: fc.cases()[n] for n in fc.SMALL}
    rc, err, got = _run(sim, str(tmp_path), cs, CLAIMS)
    assert rc == 0, (rc, err[-4000:])
    assert set(got) == set(cs)
    for name, c in cs.items():
        _hold(name, c, got[name])


def test_many_contigs(sim, tmp_path):
    c = fc.cases()["many"]
    rc, err, got = _run(sim, str(tmp_path), {"many": c}, CLAIMS)
    assert rc == 0, (rc, err[-4000:])
    _hold("many", c, got["many"])


def test_a_claim_that_is_not_met_is_reported(sim, tmp_path):
    c = fc.cases()["simple"]                                            # fewer than 64 bytes: one window
    for claim in ("windows", "header", "codes"):
        rc, err, got = _run(sim, str(tmp_path), {"one": c}, {"one": claim})
        assert rc == 4 and claim in err, (claim, rc, err[-1000:])


def test_runs_that_disagree_are_reported(sim, tmp_path):
    rc, err, got = _run(sim, str(tmp_path), {"one": fc.cases()["cut_hole"]}, {"one": "skew"})
    assert rc == 3 and "disagrees" in err, (rc, err[-1000:])


def test_a_difference_from_the_restatement_is_reported(sim, tmp_path):
    cs = fc.cases()
    for other in ("dash", "n_lower", "bad_start"):                      # another .pac; the same .pac, other holes; another status
        rc, err, got = _run(sim, str(tmp_path), {"one": cs["n_newline"]}, want={"one": cs[other]})
        assert rc == 5 and "restatement" in err, (other, rc, err[-1000:])


@pytest.mark.skipif(not refdrv.available(), reason="the reference's library (oracle/_ref) is not built")
def test_the_restatement_is_the_reference_on_well_formed_input(tmp_path):
    ref = refdrv.Ref()
    n = 0
    for name, c in fc.cases().items():
        if not c.well_formed():
            continue
        fa = str(tmp_path / (name + ".fa"))
        with open(fa, "wb") as f:
            f.write(c.text)
        assert ref.index_build(fa, fa) == 0, name
        for ext, want in (("pac", c.pac_file()), ("ann", c.ann_file()), ("amb", c.amb_file())):
            assert open(fa + "." + ext, "rb").read() == want, (name, ext)
        n += 1
    assert n >= 10

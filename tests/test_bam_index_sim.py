"""CPU test of the BAM index's device logic (arachne_amd/csrc/dev_bamindex.h): tests/baisim/bam_index_sim.cpp compiles the very functions the
kernels run, with the items of a launch in a loop, under -fsanitize=address,undefined, and is run as a plain process.  Every buffer is an
allocation of exactly its size; every case of baicases.py runs at its three slab sizes and as one slab, at seg_bytes 64, 256 and 4096, with
the items in ascending and in descending order (the program holds the 24 runs to one another); the bytes are compared with baicases.bai_of,
the serial restatement of the contract."""
import os
import subprocess

import pytest

import baicases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BI_OK, BI_E_CHAIN, BI_E_RULE, BAD_TABLE = 0, 1, 3, 4


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("baisim") / "bam_index_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "baisim", "bam_index_sim.cpp"), "-o", exe])
    return exe


def _run(sim, tmp, case):
    """-> (the program's numbers by name, the .bai's bytes or None)"""
    src, dst = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bai")
    with open(src, "wb") as f:
        f.write(case.packed())
    r = subprocess.run([sim, src, dst] + [str(s) for s in case.slabs], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    got = {l.split()[0]: int(l.split()[1]) for l in r.stdout.strip().split("\n")}
    return got, (open(dst, "rb").read() if os.path.exists(dst) else None)


def test_the_cases_are_what_they_claim():
    bc.check_cases()


@pytest.mark.parametrize("name", list(bc.cases()))
def test_index(sim, tmp_path, name):
    case = bc.cases()[name]
    got, bai = _run(sim, str(tmp_path), case)
    if case.refused is None:
        assert got["status"] == BI_OK and got["configs"] == 24 and bai == case.want
        parsed = bc.read_bai(bai)
        assert got["records"] == len(case.recs) and got["no_coor"] == parsed["n_no_coor"]
        assert got["bins"] == sum(len(r["bins"]) for r in parsed["refs"]) and got["chunks"] == sum(len(c) for r in parsed["refs"] for c in r["bins"].values())
        assert got["lin"] == sum(len(r["lin"]) for r in parsed["refs"])
        keys = [(bc.fields(r)[1], bc.reg2bin(*bc.interval(r))) for r in case.recs if bc.fields(r)[1] >= 0]
        assert got["runs"] == sum(1 for a, b in zip([None] + keys, keys) if a != b)              # whatever the slabs: a run cut by one counts once
    elif case.refused.record is None:
        assert got["status"] == BAD_TABLE and bai is None
    else:
        assert got["status"] == BI_E_RULE and bai is None
        assert (got["err"] >> 8, got["err"] & 0xff) == (case.refused.record, case.refused.rule)
    if name.startswith("slab_cuts") or name in ("one_byte_blocks", "longer_than_a_slab"):
        assert got["slabs"] >= 2


@pytest.mark.parametrize("name", list(bc.broken()))
def test_broken_chains_are_refused(sim, tmp_path, name):
    case = bc.broken()[name]
    got, bai = _run(sim, str(tmp_path), case)
    assert bai is None
    if case.refused is None:
        assert got["status"] == BI_E_CHAIN
    else:
        assert got["status"] == BI_E_RULE and (got["err"] >> 8, got["err"] & 0xff) == (case.refused.record, case.refused.rule)

"""CPU test of the CSI index's device logic (arachne_amd/csrc/dev_bamindex.h under a CSI scheme): tests/csisim/bam_index_csi_sim.cpp compiles
the very functions the kernels run, with the items of a launch in a loop, under -fsanitize=address,undefined, and is run as a plain process.
Every buffer is an allocation of exactly its size; every case of csicases.py runs at its three slab sizes and as one slab, at seg_bytes 64,
256 and 4096, with the items in ascending and in descending order (the program holds the 24 runs to one another); the inflated bytes are
compared with csicases.csi_of, the serial restatement of the contract.  The same program indexes the streams whose contigs a .bai can hold
under the BAI's scheme as well, through the same functors: those bytes are held to baicases.bai_of."""
import os
import subprocess

import pytest

import baicases as bc
import csicases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BI_OK, BI_E_CHAIN, BI_E_RULE, BAD_TABLE = 0, 1, 3, 4


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("csisim") / "bam_index_csi_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "csisim", "bam_index_csi_sim.cpp"), "-o", exe])
    return exe


def _run(sim, tmp, case, min_shift):
    """-> (the program's numbers by name, the .csi's inflated bytes or None, the .bai's bytes or None)"""
    src, dst, bai = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.csi"), os.path.join(tmp, "out.bai")
    with open(src, "wb") as f:
        f.write(cc.packed(case, min_shift))
    r = subprocess.run([sim, src, dst, bai] + [str(s) for s in case.slabs], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    got = {l.split()[0]: int(l.split()[1]) for l in r.stdout.strip().split("\n")}
    return got, (open(dst, "rb").read() if os.path.exists(dst) else None), (open(bai, "rb").read() if os.path.exists(bai) else None)


def test_the_cases_are_what_they_claim():
    queries, bounded = cc.check_cases()
    print("queries", queries, "with a non-zero lower bound", bounded)


@pytest.mark.parametrize("name", list(cc.cases()))
def test_index(sim, tmp_path, name):
    case = cc.cases()[name]
    got, csi, bai = _run(sim, str(tmp_path), case, case.min_shift)
    if case.refused is None:
        assert got["status"] == BI_OK and got["configs"] == 24 and csi == case.want
        parsed = cc.read_csi(csi)
        assert (got["min_shift"], got["depth"]) == (parsed["min_shift"], parsed["depth"]) == cc.scheme(case.min_shift, case.ref_len)
        assert got["records"] == len(case.recs) and got["no_coor"] == parsed["n_no_coor"]
        assert got["bins"] == sum(len(r["bins"]) for r in parsed["refs"]) and got["chunks"] == sum(len(c) for r in parsed["refs"] for c in r["bins"].values())
        keys = [(bc.fields(r)[1], cc.reg2bin(*bc.interval(r), parsed["min_shift"], parsed["depth"])) for r in case.recs if bc.fields(r)[1] >= 0]
        assert got["runs"] == sum(1 for a, b in zip([None] + keys, keys) if a != b)              # whatever the slabs: a run cut by one counts once
        if max(case.ref_len, default=0) <= cc.BAI_MAX:
            assert got["bai_configs"] == 24 and bai == case.bai                                  # the shared functors serve both formats
            if case.min_shift == 14:
                cc.same_as_bai(csi, case.bai)                                                    # (expected values that csi_of had no part in)
        else:
            assert got["bai_configs"] == 0 and bai is None
    elif case.refused.record is None:
        assert got["status"] == BAD_TABLE and csi is None and bai is None
    else:
        assert got["status"] == BI_E_RULE and csi is None and bai is None
        assert (got["err"] >> 8, got["err"] & 0xff) == (case.refused.record, case.refused.rule)
    if name.startswith("slab_cuts") or name in ("longer_than_a_slab", "block_size_cut"):
        assert got["slabs"] >= 2


def test_the_three_bai_cases_were_among_them():
    held = [n for n in cc.INHERITED_BAI if cc.cases()["bai_" + n].bai == bc.cases()[n].want and bc.cases()[n].want is not None]
    assert len(held) == 3


@pytest.mark.parametrize("name", list(bc.broken()))
def test_broken_chains_are_refused(sim, tmp_path, name):
    case = bc.broken()[name]
    got, csi, bai = _run(sim, str(tmp_path), case, 14)
    assert csi is None and bai is None
    if case.refused is None:
        assert got["status"] == BI_E_CHAIN
    else:
        assert got["status"] == BI_E_RULE and (got["err"] >> 8, got["err"] & 0xff) == (case.refused.record, case.refused.rule)

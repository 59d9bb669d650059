"""CPU test of the index a writer builds of what it is handed (arachne_amd/csrc/dev_bamindex.h: BiPush, the push form of bi_run over the same
slab body, with the closed form P in place of V until the block table is known): tests/bixsim/bam_index_feeds_sim.cpp compiles the very
functions the kernels run, with the items of a launch in a loop, under -fsanitize=address,undefined, and is run as a plain process.  Every
buffer is an allocation of exactly its size and every feed a copy of exactly its bytes.  Every case of baicases.py and of csicases.py is laid
out as a writer lays its file out, under file offsets of irregular steps (bixcases.py), and fed as one feed, one feed per record, and feeds of
7 and of 61 bytes, each at piece_bytes 128 and as one piece, at seg_bytes 64, 256 and 4096, the items in ascending and in descending order (the
program holds the 48 runs to one another); the bytes are compared with baicases.bai_of and csicases.csi_of over that layout.  The block-edge
cases of bixcases.edges() run the same way under their own cuttings."""
import os
import subprocess

import pytest

import baicases as bc
import bixcases as bx
import csicases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BI_OK, BI_E_CHAIN, BI_E_RULE, BAD_TABLE = 0, 1, 3, 4
PIECES = (128, 0)
CSI = [n for n in cc.cases() if cc.cases()[n].min_shift >= 0]    # (min_shift -1 is how the feeds' self-test asks for the .bai: not a .csi to refuse)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bixsim") / "bam_index_feeds_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "bixsim", "bam_index_feeds_sim.cpp"), "-o", exe])
    return exe


def _run(sim, tmp, k, groups, pieces=PIECES):
    """-> (the program's numbers by name, the index's bytes or None)"""
    src, dst, feeds = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.idx"), os.path.join(tmp, "feeds.bin")
    with open(src, "wb") as f:
        f.write(k.packed())
    with open(feeds, "wb") as f:
        f.write(bx.feeds_packed(groups))
    r = subprocess.run([sim, src, dst, str(-1 if k.min_shift is None else k.min_shift), feeds] + [str(p) for p in pieces], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    got = {l.split()[0]: int(l.split()[1]) for l in r.stdout.strip().split("\n")}
    return got, (open(dst, "rb").read() if os.path.exists(dst) else None)


def _held(k, got, out, n_groups):
    if k.refused is None:
        assert got["status"] == BI_OK and got["configs"] == 6 * len(PIECES) * n_groups and out == k.want
        assert got["records"] == len(k.recs)
    elif k.refused.record is None:
        assert got["status"] == BAD_TABLE and out is None
    else:
        assert got["status"] == BI_E_RULE and out is None
        assert (got["err"] >> 8, got["err"] & 0xff) == (k.refused.record, k.refused.rule)


def test_the_cases_are_what_they_claim():
    bx.check_edges()
    assert bx.layout(0, 0) == [] and bx.layout(5, 5) == [5] and bx.layout(65281, 65281 + 65280) == [65280, 1, 65280]
    for seed in (1, 2, 99):
        steps = [b - a for a, b in zip(bx.irregular_at(40, seed), bx.irregular_at(40, seed)[1:])]
        assert min(steps) == 26 and max(steps) == 65536 and len(set(steps)) > 20


@pytest.mark.parametrize("name", list(bc.cases()))
def test_bai(sim, tmp_path, name):
    k = bx.relaid(bc.cases()[name])
    cuts = bx.cuttings(k)
    got, out = _run(sim, str(tmp_path), k, list(cuts.values()))
    _held(k, got, out, len(cuts))
    if k.refused is None:
        keys = [(bc.fields(r)[1], bc.reg2bin(*bc.interval(r))) for r in k.recs if bc.fields(r)[1] >= 0]
        assert got["runs"] == sum(1 for a, b in zip([None] + keys, keys) if a != b)              # whatever the feeds: a run cut by one counts once


@pytest.mark.parametrize("name", CSI)
def test_csi(sim, tmp_path, name):
    case = cc.cases()[name]
    k = bx.relaid(case, case.min_shift, seed=7)
    cuts = bx.cuttings(k)
    got, out = _run(sim, str(tmp_path), k, list(cuts.values()))
    _held(k, got, out, len(cuts))


@pytest.mark.parametrize("name", list(bx.edges()))
def test_block_edges(sim, tmp_path, name):
    k = bx.edges()[name]
    cuts = bx.edge_cuttings(name, k)
    pieces = (128, 0) if name == "run_across_pieces" else (1000, 0)
    got, out = _run(sim, str(tmp_path), k, list(cuts.values()), pieces)
    assert got["status"] == BI_OK and got["configs"] == 12 * len(cuts) and out == k.want and got["records"] == len(k.recs)
    k2 = bx.Laid(k.recs, k.ref_len, k.hdr, 14, seed=3)                                           # the same stream as a .csi
    got, out = _run(sim, str(tmp_path), k2, [cuts["one"], cuts["record"]], pieces)
    assert got["status"] == BI_OK and out == k2.want


@pytest.mark.parametrize("name", list(bc.broken()))
def test_broken_chains_are_refused(sim, tmp_path, name):
    k = bx.relaid(bc.broken()[name])
    got, out = _run(sim, str(tmp_path), k, list(bx.cuttings(k).values()))
    assert out is None
    if k.refused is None:
        assert got["status"] == BI_E_CHAIN
    else:
        assert got["status"] == BI_E_RULE and (got["err"] >> 8, got["err"] & 0xff) == (k.refused.record, k.refused.rule)

"""CPU test of the device inflate's logic (arachne_amd/csrc/dev_inflate.h): tests/inflatesim/inflate_sim.cpp compiles the very functions the
kernel runs, with the lanes of a wavefront in a loop, under -fsanitize=address,undefined, and is run as a plain process.  Every block goes in
from an allocation of exactly its compressed bytes and out into one of exactly ISIZE bytes.  Every output byte and every status is compared
with what inflatecases.py computed through Python's zlib; the lanes run in ascending and in descending order."""
import os
import subprocess

import pytest

import bgzfio
import inflatecases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inflatesim") / "inflate_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "inflatesim", "inflate_sim.cpp"), "-o", exe, "-lz"])
    return exe


def _inflate(sim, tmp, chain, rev=False):
    """-> (exit status, the blocks' bytes in order, the statuses, [blocks, compressed, inflated, DEFLATE blocks])"""
    src, dst = os.path.join(tmp, "in.bgzf"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(chain)
    r = subprocess.run([sim, "inflate", src, dst] + (["rev"] if rev else []), capture_output=True, text=True)
    assert r.returncode in (0, 4), r.stderr[-4000:]
    if r.returncode == 4:
        return 4, b"", [], []
    lines = r.stdout.split("\n")
    with open(dst, "rb") as fh:
        return 0, fh.read(), [int(x) for x in lines[1].split()], [int(x) for x in lines[0].split()]


def check(case, out, status, stats, name):
    """what every run of a case must give, whoever ran it"""
    assert status == case.status, (name, status)
    offs = ic.block_offsets(case.chain)
    assert stats[0] == len(offs) and stats[1] == len(case.chain) and stats[2] == sum(n for _, n in offs) == len(out), name
    for (o, n), data, st in zip(offs, case.data, case.status):
        if st == ic.OK:
            assert out[o:o + n] == data, name
    if case.n_deflate is not None:
        assert stats[3] == case.n_deflate, name


@pytest.mark.parametrize("rev", [False, True], ids=["ascending", "descending"])
def test_good_blocks(sim, tmp_path, rev):
    for name, case in ic.good_cases().items():
        rc, out, status, stats = _inflate(sim, str(tmp_path), case.chain, rev)
        assert rc == 0, name
        check(case, out, status, stats, name)


@pytest.mark.parametrize("rev", [False, True], ids=["ascending", "descending"])
def test_damaged_blocks_give_their_status_and_leave_the_neighbours_alone(sim, tmp_path, rev):
    seen = set()
    for name, case in ic.damage_cases().items():
        rc, out, status, stats = _inflate(sim, str(tmp_path), case.chain, rev)
        assert rc == 0, name
        check(case, out, status, stats, name)
        seen.add(case.status[1])
    assert seen == set(range(1, 10))              # one case per status at least
    for name, chain in ic.untiled_chains().items():
        assert _inflate(sim, str(tmp_path), chain, rev)[0] == 4, name


def test_the_cases_are_what_they_claim():
    """asserted from the streams themselves, parsed by inflatecases.scan"""
    good = ic.good_cases()
    assert all(b["btype"] == 0 for b in ic.structure("stored_level0")) and all(b["btype"] == 0 for b in ic.structure("stored_random_65280"))
    assert [b["btype"] for b in ic.structure("fixed_text")] == [1]
    for level in (1, 4, 6, 9):
        assert all(b["btype"] == 2 for b in ic.structure("dynamic_level%d" % level))
    assert len(ic.structure("dynamic_memlevel1")) >= 50                           # many DEFLATE blocks inside one BGZF block
    flushes = ic.structure("dynamic_flushes")
    empty = [b for k, b in enumerate(flushes) if b["btype"] == 0]
    assert len(empty) == 3 and any((b["bitpos"] + 3) % 8 for b in empty)              # empty stored blocks, not all byte-aligned
    assert max(ic.structure("fifteen_bit_codes")[0]["ll_lens"]) == 15
    nd = ic.structure("no_distance_code")[0]
    assert nd["hdist"] == 1 and nd["d_lens"] == [0]
    sd = ic.structure("single_distance_code")[0]
    assert [l for l in sd["d_lens"] if l] == [1]
    cross = ic.structure("run_across_the_border")[0]
    assert cross["crossing"] and not any(b.get("crossing") for b in ic.structure("dynamic_level6"))
    assert [b["isize"] for b in bgzfio.split(good["isize_0_in_the_middle_and_at_the_end"].chain)] == [300, 0, 600, 0]
    assert bgzfio.split(good["full_block_65536"].chain)[0]["isize"] == 65536
    assert len(bgzfio.split(good["three_hundred_blocks"].chain)) == 300
    far = ic.structure("distance_32768")
    assert [b["btype"] for b in far] == [0, 1] and far[1]["max_dist"] == 32768 and far[1]["n_matches"] == 2       # the window's edge
    assert ic.structure("match_ends_on_last_byte")[-1]["ends_in_match"]
    assert good["run_of_one_byte"].data[0] == b"a" * 65280

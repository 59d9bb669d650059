"""CPU test of the search for block starts of the chunked gzip inflate (arachne_amd/csrc/dev_gunzip.h): gz_find, the stated reference form (64
positions a round), against gz_find_runs, which gz_chunk_find calls (a run of positions per lane behind a prefilter on the 13 header bits that
need no table).  tests/gzfindsim/gzfind_sim.cpp compiles both for the host under -fsanitize=address,undefined, runs them on every chunk's range
of a file, lanes ascending and descending, and exits non-zero where any chunk's position differs.  Inputs: every stream of gunzipcases.cases()
and the pair of tests/test_feeder_gunzip.py, at chunks of 64, 4,096 and 32,768 bytes; and two constructed ranges.  (tests/test_gunzip_sim.py
and tests/test_gunzip_gpu.py pin the bytes and the statistics through the new search.)"""
import gzip
import os
import subprocess

import pytest

import fqstdcases as sc
import gunzipcases as gc
import inflatecases as ic
import test_feeder_gunzip as tfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (64, 4096, 32768)
PIECE = 2048                     # dev_gunzip.h: GZ_PIECE


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("gzfindsim")), "gzfind_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "gzfindsim", "gzfind_sim.cpp"), "-o", exe])
    return exe


def run(sim, tmp, data, chunk, rev=False):
    """-> [(cand, positions in front of it that pass the prefilter, ... that pass gz_cheap)] per chunk; the program's exit status is asserted"""
    src = os.path.join(str(tmp), "in.bin")
    with open(src, "wb") as f:
        f.write(data)
    r = subprocess.run([sim, src, str(chunk)] + (["rev"] if rev else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]               # 3: the two forms differ on a chunk
    return [tuple(int(x) for x in line.split()[1:]) for line in r.stdout.splitlines()]


def test_both_forms_find_the_same_position_on_every_chunk(sim, tmp_path):
    streams = {name: case.data for name, case in gc.cases().items()}
    t1, t2 = (tfg._random_reads(t, 31 + k) for k, t in enumerate(sc.raw_pair(sc.HAPLOTAGGING, 1500, seed=9, l1=100, l2=90)[:2]))
    streams.update(pair_r1=gzip.compress(t1, 6), pair_r2=gzip.compress(t2, 6), pair_r1_mem5=gc.gz(t1, 6, tfg.MEM))
    found = 0
    for name, data in streams.items():
        for chunk in CHUNKS:
            up = run(sim, tmp_path, data, chunk)
            assert run(sim, tmp_path, data, chunk, rev=True) == up, (name, chunk)
            found += sum(c[0] >= 0 for c in up)
    assert found > 1000                                      # the searches had something to find


def _block(w):
    ic.dynamic_block(gc._letters(40), gc.LL, gc.D_FAR, final=False, w=w)
    ic.fixed_block(gc._letters(5, 1), final=True, w=w)
    return w.bytes()


def test_the_only_candidate_on_the_last_position_of_a_piece(sim, tmp_path):
    """zero bits pass nowhere (BTYPE 0); a dynamic block starts at bit 8 * GZ_PIECE - 1, the last position of the first piece and of the last
    lane's run, its header in the next piece"""
    w = ic.BitWriter()
    w.put(0, 8 * PIECE - 1)
    data = _block(w)
    for rev in (False, True):
        assert run(sim, tmp_path, data, PIECE, rev)[0] == (8 * PIECE - 1, 0, 0)
        assert run(sim, tmp_path, data, 4 * PIECE, rev)[0] == (8 * PIECE - 1, 0, 0)


@pytest.mark.parametrize("at", [1000, 32 * 8 - 3, 8 * PIECE - 3])
def test_a_block_start_behind_a_position_that_fails_the_kraft_sum(sim, tmp_path, at):
    """Position `at` reads BFINAL 0, BTYPE 2, HLIT 4 + ... <= 29, HDIST <= 29 and code length code lengths whose Kraft sum is not one; the true
    block starts 3 bits behind it.  (Not 1 or 2 bits: the position in front of a non-final dynamic block's start reads its BTYPE from the
    start's BFINAL 0 and first BTYPE bit 0, the one before that its second BTYPE bit from BFINAL -- neither can read BTYPE 2.)  `at`: in the
    middle of a lane's run, with the start in the next lane's run, and with the start in the next piece"""
    w = ic.BitWriter()
    w.put(0, at)
    w.put(4, 3)                                              # BFINAL 0, BTYPE 2 as position `at` reads them
    data = _block(w)
    for rev in (False, True):
        assert run(sim, tmp_path, data, 4 * PIECE, rev)[0] == (at + 3, 1, 0)    # one position passed the prefilter, none gz_cheap

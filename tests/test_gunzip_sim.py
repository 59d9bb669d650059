"""CPU test of the chunked gzip inflate (arachne_amd/csrc/dev_gunzip.h, gunzip_host.h): tests/gunzipsim/gunzip_sim.cpp compiles the very
functions the kernels run and the reader that drives them, with the lanes of a wavefront and the wavefronts of a launch in a loop, under
-fsanitize=address,undefined, and is run as a plain process.  Inside the program every case is compared with zlib's gzread of the same file:
the bytes, and whether an error is reported.  Here the bytes are compared with Python's zlib, member by member, and the statistics with what
the case states; lanes and wavefronts run in ascending and in descending order."""
import pytest

import gunzipcases as gc
import inflatecases as ic


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return gc.build_sim(str(tmp_path_factory.mktemp("gunzipsim")))


@pytest.fixture(scope="module")
def results(sim, tmp_path_factory):
    """every case through the host twin, lanes ascending: run once, shared"""
    tmp = str(tmp_path_factory.mktemp("gunzip_runs"))
    return {name: gc.run_sim(sim, tmp, case) for name, case in gc.cases().items()}


def test_every_case_reads_what_gzread_reads(results):
    for name, case in gc.cases().items():
        gc.check(case, results[name], name)


def test_descending_lanes_and_wavefronts_give_the_same(sim, tmp_path, results):
    for name, case in gc.cases().items():
        res = gc.run_sim(sim, str(tmp_path), case, rev=True)
        gc.check(case, res, name)
        assert {k: res[k] for k in gc.STATS} == {k: results[name][k] for k in gc.STATS}, name


def test_the_forced_fallbacks_give_their_reasons(results):
    assert results["block_larger_than_a_slab"]["fallback"] == gc.FB_NO_BLOCK
    r = results["gzip_inside_stored_blocks"]
    assert r["fallback"] == gc.FB_REFUTED and r["refuted"] >= 1
    assert results["overflow"]["fallback"] == gc.FB_OVERFLOW
    r = results["thirty_tiny_members"]
    assert r["fallback"] == gc.FB_CUT_SHORT and r["members"] == 30 and r["launches"] == 2
    r = results["damage_flipped_bit_in_a_late_chunk"]
    assert r["rc"] == gc.ARX_E_IO


def test_the_cases_are_what_they_claim(results):
    """asserted from the streams themselves, parsed by inflatecases.scan, and from the host twin's counts"""
    c = gc.cases()
    for level in (1, 6, 9):
        blocks = gc.deflate_blocks(c["level%d_chunk4096" % level].data)
        assert all(b["btype"] == 2 for b in blocks) and len(blocks) >= 3
        assert results["level%d_chunk4096" % level]["accepted"] >= 3                     # more than one chunk took part
    many = gc.deflate_blocks(c["memlevel1_chunk4096"].data)
    assert len(many) >= 100                                                              # a block every few hundred bytes
    r = results["memlevel1_chunk4096"]
    assert r["inflated_bytes"] < 32768 * r["accepted"] and r["markers"] > 0              # a chunk of fewer than 32768 symbols: its window mixes two
    r = results["chunk_below_the_block_spacing"]
    assert r["candidates"] * 4 < r["chunks"] and r["accepted"] >= 2                      # most chunks have none, and a chunk crosses several ranges
    far = gc.deflate_blocks(gc.distance_32768()[0])
    assert [b["btype"] for b in far] == [0, 2, 1] and far[1]["max_dist"] == 32768 and far[1]["n_matches"] == 2
    r = results["distance_32768"]
    assert r["accepted"] == 2 and r["markers"] == 261                                    # the matches' source lies in the chunk before
    text, motif = gc.motif_text()
    blocks = gc.deflate_blocks(c["motif_through_many_windows"].data)
    assert sum(1 for b in blocks if b["btype"] == 2 and b["max_dist"] > 16000) >= 10 and text.count(motif) == 15
    r = results["motif_through_many_windows"]
    assert r["accepted"] >= 10 and r["markers"] >= 10 * len(motif)
    r = results["marker_across_a_launch"]
    assert r["launches"] >= 4 and r["markers"] > 0
    ring = gc.deflate_blocks(gc.ring_hazard()[0])
    assert [b["btype"] for b in ring] == [0, 2, 1] and ring[1]["max_dist"] == 32768 and ring[1]["n_matches"] == 7
    assert results["ring_hazard"]["accepted"] == 1                                       # one decoder, one ring
    run = gc.deflate_blocks(gc.run_of_one_byte()[0])
    assert all(b["max_dist"] == 1 for b in run[:-1]) and len(run) == 13
    r = results["run_of_one_byte"]
    assert r["accepted"] >= 4 and r["markers"] > 258 * 200
    assert all(b["btype"] == 0 for b in gc.deflate_blocks(c["level0_stored_only"].data))
    r = results["level0_stored_only"]
    assert r["candidates"] == 1 and r["accepted"] == 1 and r["chunks"] > 20              # no candidate anywhere: chunk 0 crosses the whole slab
    assert all(b["btype"] == 1 for b in gc.deflate_blocks(c["z_fixed"].data))
    flushes = gc.deflate_blocks(c["flushes"].data)
    empty = [b for b in flushes if b["btype"] == 0]
    assert len(empty) == 5 and any((b["bitpos"] + 3) % 8 for b in empty)                 # empty stored blocks, not all byte-aligned
    assert gc.deflate_blocks(c["level6_chunk4096"].data)[-1]["btype"] == 2 and ring[-1]["btype"] == 1           # the final block: dynamic, fixed, stored
    assert gc.deflate_blocks(c["level0_stored_only"].data)[-1]["btype"] == 0
    assert results["five_members"]["members"] == 5 and results["two_members_small_slabs"]["launches"] >= 6
    for name in ("empty_member_first", "empty_member_in_the_middle", "empty_member_last"):
        assert results[name]["members"] == 3
    assert results["trailing_zeros"]["ignored_bytes"] == 100 and results["lone_1f_at_the_end"]["ignored_bytes"] == 1
    assert results["trailing_bytes"]["ignored_bytes"] == len(b"no gzip header here, \x1f\x8b or not")
    on = c["member_end_on_a_chunk_boundary"].data
    assert len(on) == 2 * (10 + 128 + 8)
    assert results["slab_end_inside_a_stored_len"]["launches"] >= 2
    inner = gc.deflate_blocks(c["level6_chunk4096"].data)
    assert sum(1 for b in inner if b["btype"] == 2) >= 3                                 # true dynamic headers inside the stored bytes of the outer file


def test_scan_reads_what_zlib_reads():
    for name in ("level6_chunk4096", "memlevel1_chunk4096", "flushes", "motif_through_many_windows"):
        m = gc.cases()[name].data
        assert ic.scan(gc.body_of(m))[0] == gc.expected(m)[0], name

"""The device feeder on BGZF input with the inflate on the device (arx_feeder_open_device_ex, ARX_FEEDER_INFLATE_DEVICE: csrc/feeder.h
BgzfChunkReader, device_feeder.h, dev_inflate.h).  The pin is the host feeder (arx_feeder_open) on the PLAIN files: the super-batches are
byte for byte the same, whatever the blocks' sizes, wherever the cuts between parses fall.  The BGZF files are written by tests/bgzfio.py
(Python's zlib).  Every test exists twice: on the host test double, where dev_inflate.h's functions run with the lanes in a loop, and on the
product library (-m gpu)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import bgzfio
import devfeed
from devfeed import SIM
from arachne_amd import api, synth

LIBS = [pytest.param("sim", id="hostsim"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
_REFS = {}


@pytest.fixture(scope="module")
def libs(built):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    yield {"sim": SIM, "gpu": api.LIB_PATH}
    for r in _REFS.values():
        r.close()
    _REFS.clear()


def _ref(lib_path):
    if lib_path not in _REFS:
        d = tempfile.mkdtemp(prefix="arx_bgzfeed_ref_")
        fa = os.path.join(d, "g.fa")
        synth.make_genome(3, [20000, 6000]).write_fasta(fa)
        api.index_build(fa, fa, lib_path=lib_path)
        _REFS[lib_path] = api.Reference(fa, lib_path=lib_path)
    return _REFS[lib_path]


def device_batches(lib_path, p1, p2, target, chunk_bytes=0, parse_chunks=None, inflate="device"):
    """-> (snapshots of every super-batch, the feeder's stats)"""
    old = os.environ.pop("ARX_FEEDER_PARSE_CHUNKS", None)
    if parse_chunks:
        os.environ["ARX_FEEDER_PARSE_CHUNKS"] = str(parse_chunks)
    try:
        fd = api.Feeder(p1, p2, device=_ref(lib_path), chunk_bytes=chunk_bytes, inflate=inflate)
    finally:
        os.environ.pop("ARX_FEEDER_PARSE_CHUNKS", None)
        if old is not None:
            os.environ["ARX_FEEDER_PARSE_CHUNKS"] = old
    out = devfeed.feed_all(fd, target)
    st = fd.stats()
    fd.close()
    return out, st


def host_batches(lib_path, p1, p2, target):
    fd = api.Feeder(p1, p2, lib_path=lib_path)
    out = devfeed.feed_all(fd, target)
    fd.close()
    return out


def same_batches(got, want):
    """devfeed.assert_same_batches's comparison: every array of every super-batch, byte for byte"""
    assert len(got) == len(want), (len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.keys() == b.keys()
        for key in a:
            assert a[key] == b[key], (k, key)


def chunks_of(sizes, chunk):
    """the documented rule: a chunk is the longest run of whole blocks that inflate to at most chunk bytes, at least one block
    -> the offsets of the text at which a new chunk starts (without 0)"""
    starts, at, run, open_ = [], 0, 0, False
    for n in sizes:
        if open_ and run + n > chunk:
            starts.append(at)
            run, open_ = 0, False
        run += n
        at += n
        open_ = True
    return starts


def random_cuts(n, rng, lo=1, hi=300):
    cuts, at = [], 0
    while True:
        at += int(rng.integers(lo, hi + 1))
        if at >= n:
            return cuts
        cuts.append(at)


def sizes_of(n, cuts):
    return [b - a for a, b in bgzfio.cut_points(n, cuts)]


TEXT_GROUPS = [("A-1", 3), ("B-1", 260), ("C", 7), (None, 2), ("D-1", 330), ("E-1", 1), ("F-1", 197)]


@pytest.fixture(scope="module")
def texts():
    t1, t2 = devfeed.fastq(TEXT_GROUPS, seed=4)
    return t1.encode("latin-1"), t2.encode("latin-1")[:-1]          # R2 without its last newline


@pytest.fixture(scope="module")
def plain(libs, texts):
    """the plain files, and what the host feeder delivers for them (computed once per library)"""
    d = tempfile.mkdtemp(prefix="arx_bgzfeed_")
    p1, p2 = devfeed.write(d, "r1.fq", texts[0]), devfeed.write(d, "r2.fq", texts[1])
    want = {}

    def get(which):
        if which not in want:
            want[which] = host_batches(libs[which], p1, p2, 100)
        return want[which]
    return d, p1, p2, get


@pytest.mark.parametrize("which", LIBS)
def test_blocks_of_1_to_300_bytes_one_chunk_per_parse(libs, which, texts, plain):
    """chunk_bytes = 64 and a parse per chunk: a cut between two parses falls at every offset inside a record (asserted from the cut points
    and the texts), each of them in mid-line of one file while the other file's cut is somewhere else"""
    d, _, _, want = plain
    rng = np.random.default_rng(17)
    cuts = [random_cuts(len(t), rng) for t in texts]
    paths = [os.path.join(d, "tiny_r%d.fq.gz" % (f + 1)) for f in range(2)]
    for f in range(2):
        bgzfio.write_bgzf_file(paths[f], texts[f], cut=cuts[f], level=1 + 4 * f, eof=bool(f))
    starts = [chunks_of(sizes_of(len(t), c), 64) for t, c in zip(texts, cuts)]
    seen = set()
    for t, st in zip(texts, starts):
        heads = np.array([m for m in range(len(t)) if t.startswith(b"@read", m) and (m == 0 or t[m - 1] == 10)])
        at = np.array(st)
        seen |= set((at - heads[np.searchsorted(heads, at, side="right") - 1]).tolist())
    shortest = min(len(r) for t in texts for r in t.split(b"@read")[1:-1]) + 5
    assert set(range(shortest)) <= seen                          # every offset of a record, a cut between parses
    got, st = device_batches(libs[which], paths[0], paths[1], 100, chunk_bytes=64, parse_chunks=1)
    same_batches(got, want(which))
    n_blocks = [len(c) + 1 for c in cuts]
    assert st["device_blocks"] == n_blocks[0] + n_blocks[1] + 1      # R2 has its EOF block
    assert st["compressed_bytes"] == os.path.getsize(paths[0]) + os.path.getsize(paths[1])
    assert st["bytes"] == len(texts[0]) + len(texts[1]) and st["fallback_chunks"] == 0
    # (the EOF block is a block like any other: a chunk of its own behind a block of more than 64 bytes)
    assert st["chunks"] == len(starts[0]) + 1 + len(chunks_of(sizes_of(len(texts[1]), cuts[1]) + [0], 64)) + 1
    # without the flag the same files go through zlib on the reader threads: the same super-batches, nothing on the device
    got0, st0 = device_batches(libs[which], paths[0], paths[1], 100, chunk_bytes=64, inflate="host")
    same_batches(got0, want(which))
    assert st0["device_blocks"] == 0 and st0["compressed_bytes"] == 0 and st0["bytes"] == st["bytes"]


FORMS = ["blocks_65280", "mixed", "r2_gzip", "r2_plain", "no_eof_block", "eof_block_in_the_middle"]


@pytest.mark.parametrize("which", LIBS)
@pytest.mark.parametrize("form", FORMS)
def test_plain_against_bgzf(libs, which, form, texts, plain):
    d, p1, p2, want = plain
    rng = np.random.default_rng(FORMS.index(form))
    paths = [os.path.join(d, "%s_r%d.fq.gz" % (form, f + 1)) for f in range(2)]
    n_blocks = n_bytes = 0
    chunk = 4096
    for f, t in enumerate(texts):
        if f == 1 and form == "r2_gzip":
            paths[1] = devfeed.write(d, "r2_ordinary.fq.gz", t, gz=True)
            continue
        if f == 1 and form == "r2_plain":
            paths[1] = p2
            continue
        if form == "blocks_65280":
            cut, chunk = bgzfio.BLOCK_IN, 0
            assert len(t) > 65280
        elif form == "mixed":
            cut = sorted(set(random_cuts(len(t) // 2, rng, 1, 40) + [len(t) // 2] + random_cuts(len(t), rng, 20000, 65280)))
        elif form == "eof_block_in_the_middle":
            cut = random_cuts(len(t), rng, 500, 9000)
            cut = sorted(cut + cut[2:4])                          # two empty blocks: the form of the EOF block, not at the end
        else:
            cut = random_cuts(len(t), rng, 500, 9000)
        raw = bgzfio.write_bgzf_file(paths[f], t, cut=cut, level=4, eof=form != "no_eof_block")
        blocks = bgzfio.split(raw)
        if form == "eof_block_in_the_middle":
            assert [b["isize"] for b in blocks].count(0) == 3 and blocks[3]["isize"] == 0
        n_blocks += len(blocks)
        n_bytes += len(raw)
    got, st = device_batches(libs[which], paths[0], paths[1], 100, chunk_bytes=chunk)
    same_batches(got, want(which))
    assert st["device_blocks"] == n_blocks and st["compressed_bytes"] == n_bytes
    assert st["bytes"] == len(texts[0]) + len(texts[1]) and st["fallback_chunks"] == 0


@pytest.mark.parametrize("which", LIBS)
def test_damaged_text_seeded(libs, which):
    """100 of devfeed.damaged_pair's files in their BGZF form, blocks of 1 to 300 bytes: equal to the host feeder on the plain files"""
    lib = libs[which]
    d = tempfile.mkdtemp(prefix="arx_bgzfeed_")
    rng = np.random.default_rng(5)
    for seed in range(100):
        t1, t2, _ = devfeed.damaged_pair(seed)
        b1, b2 = t1.encode("latin-1"), t2.encode("latin-1")
        want = host_batches(lib, devfeed.write(d, "r1.fq", b1), devfeed.write(d, "r2.fq", b2), 7)
        z1, z2 = os.path.join(d, "r1.fq.gz"), os.path.join(d, "r2.fq.gz")
        bgzfio.write_bgzf_file(z1, b1, cut=random_cuts(len(b1), rng), eof=bool(seed & 1))
        bgzfio.write_bgzf_file(z2, b2, cut=random_cuts(len(b2), rng), eof=bool(seed & 2))
        got, st = device_batches(lib, z1, z2, 7, chunk_bytes=64, parse_chunks=1 if seed % 4 == 0 else None)
        same_batches(got, want)
        assert 0 < st["bytes"] <= len(b1) + len(b2) and st["device_blocks"] > 0, seed   # the input ends where the shorter file does


@pytest.mark.parametrize("which", LIBS)
def test_a_file_of_an_eof_block_alone_is_the_end_of_the_input(libs, which):
    d = tempfile.mkdtemp(prefix="arx_bgzfeed_")
    p = [devfeed.write(d, "r%d.fq.gz" % f, bgzfio.EOF_BLOCK) for f in (1, 2)]
    got, st = device_batches(libs[which], p[0], p[1], 10)
    assert [sb["n_sets"] for sb in got] == [0] and st["device_blocks"] == 2 and st["bytes"] == 0 and st["records"] == 0


def _until_error(fd, target):
    out = []
    while True:
        sb = api._SuperBatch()
        n = fd.lib.arx_feeder_next(fd.h, int(target), C.byref(sb))
        if n <= 0:
            return out, n
        out.append(devfeed.snapshot(sb, n))


@pytest.mark.parametrize("which", LIBS)
@pytest.mark.parametrize("damage", ["crc", "stream", "not_bgzf", "bsize_past_the_end"])
def test_a_damaged_block_in_mid_file_ends_the_input_like_a_read_error(libs, which, damage, texts):
    """R1's block k is damaged.  What arrives is what the host feeder delivers for R1 cut in front of that block, except that the end is a
    read error: the last set, which the end cut short, is not flagged unique (device_feeder.h: next()), and the call after it fails"""
    lib = libs[which]
    t1, t2 = texts
    d = tempfile.mkdtemp(prefix="arx_bgzfeed_")
    cut = random_cuts(len(t1), np.random.default_rng(9), 2000, 5000)
    raw = bgzfio.write_bgzf(t1, cut=cut, level=4)
    blocks = bgzfio.split(raw)
    k = len(blocks) // 2
    b = blocks[k]
    text_before = sum(x["isize"] for x in blocks[:k])
    if damage == "crc":
        bad = raw[:b["at"] + b["size"] - 8] + bytes([raw[b["at"] + b["size"] - 8] ^ 1]) + raw[b["at"] + b["size"] - 7:]
    elif damage == "stream":
        mid = b["at"] + 18 + len(b["payload"]) // 2
        bad = raw[:mid] + bytes([raw[mid] ^ 0x55, raw[mid + 1] ^ 0xAA]) + raw[mid + 2:]
    elif damage == "not_bgzf":
        bad = raw[:b["at"]] + b"@not a block\n" + raw[b["at"]:]
    else:
        bad = raw[:b["at"] + b["size"] // 2]
    p1, p2 = devfeed.write(d, "r1.fq.gz", bad), devfeed.write(d, "r2.fq", t2)
    want = host_batches(lib, devfeed.write(d, "cut_r1.fq", t1[:text_before]), p2, 10**6)
    assert len(want) == 2 and want[0]["n_sets"] >= 3
    for chunk in (0, 4096):
        fd = api.Feeder(p1, p2, device=_ref(lib), chunk_bytes=chunk, inflate="device")
        got, rc = _until_error(fd, 10**6)
        assert rc < 0 and fd.lib.arx_feeder_next(fd.h, 10, C.byref(api._SuperBatch())) < 0      # and it stays an error
        assert fd.stats()["bytes"] >= text_before
        fd.close()
        assert len(got) == 1
        for key in want[0]:
            if key in ("unique", "do_rfa"):
                assert got[0][key][:-1] == want[0][key][:-1] and got[0][key][-1] == 0, key
            else:
                assert got[0][key] == want[0][key], key


@pytest.mark.parametrize("which", LIBS)
def test_unknown_flag_bits_are_refused(libs, which, plain):
    _, p1, p2, _ = plain
    ref = _ref(libs[which])
    h, msg = C.c_void_p(), C.create_string_buffer(256)
    for flags in (2, 3, -1, 1 << 20):
        assert ref.lib.arx_feeder_open_device_ex(ref.h, p1.encode(), p2.encode(), 0, 1, flags, C.byref(h), msg, 256) == -2 and not h.value
        assert b"flag" in msg.value
    with pytest.raises(ValueError):
        api.Feeder(p1, p2, lib_path=libs[which], inflate="device")            # the host feeder has no device inflate

"""The device feeder on ordinary gzip input with the inflate on the device (arx_feeder_open_device_ex, ARX_FEEDER_GUNZIP_DEVICE: csrc/device_feeder.h,
gunzip_host.h, dev_gunzip.h).  The pin is the host feeder (arx_feeder_open) on the PLAIN files: the super-batches are byte for byte the same,
whatever the chunk, the slab and the parse-chunk setting.  The text has random bases and qualities (text that compresses thirty times shows
nothing); ARX_FEEDER_GUNZIP_CHUNK=4096 and ARX_FEEDER_GUNZIP_SLAB=16384 put a dozen chunks and four launches into each file of 47 to 59 KB.
zlib at its default memLevel of 8 ends a block of this text every 24 KB, so that no block ends inside a slab of 16 KiB and the reference inflate
alone hands such a file to the host (NO_BLOCK) whatever the seed; the streams of the four forms are therefore written with memLevel 5 (a block
every 4 KB), which is gzip of the stated levels all the same.  Files as gzip.compress writes them (memLevel 8) go through at the defaults and
with slabs of 32 KiB in a form of their own.
Every test exists twice: on the host test double, where dev_gunzip.h's functions run with lanes and chunks in a loop, and on the product
library (-m gpu)."""
import ctypes as C
import gzip
import os
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

import bgzfio
import devfeed
import fqstdcases as sc
import gunzipcases as gc
from devfeed import SIM
from arachne_amd import api, synth

LIBS = [pytest.param("sim", id="hostsim"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
TARGETS = (1, 77, 400, 10**6)
SMALL = dict(gz_chunk=4096, gz_slab=16384, parse_chunks=1)
SMALL_MEM8 = dict(gz_chunk=4096, gz_slab=32768, parse_chunks=1)
SWITCHES = dict(gz_chunk="ARX_FEEDER_GUNZIP_CHUNK", gz_slab="ARX_FEEDER_GUNZIP_SLAB", parse_chunks="ARX_FEEDER_PARSE_CHUNKS")
ARX_E_ARG = -2
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
        d = tempfile.mkdtemp(prefix="arx_gzfeed_ref_")
        fa = os.path.join(d, "g.fa")
        synth.make_genome(3, [20000, 6000]).write_fasta(fa)
        api.index_build(fa, fa, lib_path=lib_path)
        _REFS[lib_path] = api.Reference(fa, lib_path=lib_path)
    return _REFS[lib_path]


def _random_reads(text, seed):
    """the same records with random bases and qualities of the same lengths (test_fastq_gunzip_gpu.py's recipe)"""
    rng = np.random.default_rng(seed)
    lines = text.split(b"\n")
    for k in range(1, len(lines), 4):
        n = len(lines[k])
        lines[k] = bytes(b"ACGT"[i] for i in rng.integers(0, 4, n))
        lines[k + 2] = bytes(int(q) for q in np.array([35, 45, 56, 70], np.uint8)[rng.choice(4, n, p=[.02, .05, .13, .8])])
    return b"\n".join(lines)


MEM = 5                          # zlib's memLevel of the forms' streams: 2,048 symbols a block


def _members(t):
    cut = (len(t) // 2 + 17, len(t) // 2 + 17 + len(t) // 3)
    return gc.gz(t[:cut[0]], 1, MEM) + gc.gz(t[cut[0]:cut[1]], 9, MEM) + gc.gz(t[cut[1]:], 6, MEM)


def open_feeder(lib_path, p1, p2, chunk_bytes=0, gunzip="device", inflate="host", **sw):
    """a device feeder opened with the switches of `sw` set (gz_chunk, gz_slab, parse_chunks) and nothing of them left behind"""
    old = {v: os.environ.pop(v, None) for v in SWITCHES.values()}
    for k, v in sw.items():
        os.environ[SWITCHES[k]] = str(v)
    try:
        return api.Feeder(p1, p2, device=_ref(lib_path), chunk_bytes=chunk_bytes, gunzip=gunzip, inflate=inflate)
    finally:
        for v in SWITCHES.values():
            os.environ.pop(v, None)
            if old[v] is not None:
                os.environ[v] = old[v]


def device_batches(lib_path, p1, p2, target, **kw):
    """-> (snapshots of every super-batch, the two files' gunzip_stats, the feeder's stats)"""
    fd = open_feeder(lib_path, p1, p2, **kw)
    out = devfeed.feed_all(fd, target)
    gs, st = fd.gunzip_stats(), fd.stats()
    fd.close()
    return out, gs, st


def host_batches(lib_path, p1, p2, target):
    fd = api.Feeder(p1, p2, lib_path=lib_path)
    out = devfeed.feed_all(fd, target)
    fd.close()
    return out


ZERO = {k: 0 for k in api.GUNZIP_STATS}


def taken(gs, members):
    """the device was given this file and took all of it"""
    assert gs["launches"] >= 1 and gs["accepted"] >= gs["launches"] and gs["host_bytes"] == 0 and gs["fallback"] == 0 and gs["members"] == members, gs


@pytest.fixture(scope="module")
def texts():
    t1, t2 = (_random_reads(t, 31 + k) for k, t in enumerate(sc.raw_pair(sc.HAPLOTAGGING, 1500, seed=9, l1=100, l2=90)[:2]))
    return t1, t2


@pytest.fixture(scope="module")
def files(libs, texts, tmp_path_factory):
    """the plain pair, its forms, and per library what the host feeder delivers for the plain pair (computed once per library and target).
    Each gzip file is shown first to stay inside what the reference inflate takes alone, at the sizes the tests use: the statistics the tests
    assert are then a cap on what the feeder may skip, not a wish"""
    d = str(tmp_path_factory.mktemp("gzfeed"))
    plain = [devfeed.write(d, "r%d.fq" % (f + 1), t) for f, t in enumerate(texts)]
    data = dict(gzip=[gc.gz(t, 6, MEM) for t in texts], members=[_members(t) for t in texts], mem8=[gzip.compress(t, 6) for t in texts])
    forms = {}
    for name, both in data.items():
        forms[name] = [devfeed.write(d, "%s_r%d.fq.gz" % (name, f + 1), z) for f, z in enumerate(both)]
        assert all(len(z) > 40000 for z in both)
    forms["r2_plain"] = [forms["gzip"][0], plain[1]]
    forms["r1_bgzf"] = [os.path.join(d, "bgzf_r1.fq.gz"), forms["gzip"][1]]
    bgzfio.write_bgzf_file(forms["r1_bgzf"][0], texts[0], cut=bgzfio.BLOCK_IN, level=4, eof=True)
    want, shown = {}, set()

    def host(which, target):
        if (which, target) not in want:
            want[which, target] = host_batches(libs[which], plain[0], plain[1], target)
        return want[which, target]

    def show(which):
        """the reference inflate alone on every gzip file, defaults and the small sizes: no fallback"""
        if which in shown:
            return
        shown.add(which)
        sim = gc.build_sim(d, sanitize=False) if which == "sim" else None
        for name, both in data.items():
            for z in both:
                for chunk, slab in ((0, 0), (4096, 32768 if name == "mem8" else 16384)):
                    if which == "sim":
                        r = gc.run_sim(sim, d, gc.Case(z, chunk, slab, 0, True, gc.FB_NONE, gc.ARX_OK))
                    else:
                        r = api.selftest_gunzip(z, chunk_bytes=chunk, slab_bytes=slab, cap=1 << 20)
                    assert r["rc"] == 0 and r["fallback"] == 0 and r["host_bytes"] == 0 and r["members"] == (3 if name == "members" else 1), (name, chunk, r)
                    if chunk and name != "mem8":
                        assert r["chunks"] >= 12 and r["launches"] >= 4, r
    return dict(d=d, plain=plain, forms=forms, host=host, show=show)


FORMS = dict(gzip=(8, (1, 1)), members=(8, (3, 3)), r2_plain=(8, (1, None)), r1_bgzf=(9, (None, 1)), mem8=(8, (1, 1)))     # flags, members per file (None: not the device's gunzip)


@pytest.mark.parametrize("which", LIBS)
@pytest.mark.parametrize("form", list(FORMS))
def test_super_batches_are_the_host_feeders(libs, which, form, files):
    """cases 1 and 2: every form at the defaults and at the small chunk / slab with a parse per chunk, chunk_bytes 4,096 and 50,000 (ragged
    against the text: parse cuts fall everywhere); the device took every gzip file whole and was given no other"""
    files["show"](which)
    p1, p2 = files["forms"][form]
    flags, members = FORMS[form]
    inflate = "device" if flags & 1 else "host"
    small = SMALL_MEM8 if form == "mem8" else SMALL
    for kw in (dict(), dict(chunk_bytes=4096, **small), dict(chunk_bytes=50000, **small)):
        for target in TARGETS:
            got, gs, st = device_batches(libs[which], p1, p2, target, inflate=inflate, **kw)
            devfeed.assert_same_batches(got, files["host"](which, target))
            for f in range(2):
                if members[f] is None:
                    assert gs[f] == ZERO, (form, f, gs[f])
                else:
                    taken(gs[f], members[f])
                    if kw:
                        assert (gs[f]["launches"] >= 2 and gs[f]["chunks"] >= 12) if form == "mem8" else (gs[f]["launches"] >= 4 and gs[f]["chunks"] >= 12), gs[f]
            assert st["fallback_chunks"] == 0 and st["bytes"] == sum(os.path.getsize(p) for p in files["plain"])
            assert (st["device_blocks"] > 0) == (form == "r1_bgzf")


@pytest.mark.parametrize("which", LIBS)
def test_without_the_flag_nothing_goes_to_the_device(libs, which, files):
    p1, p2 = files["forms"]["gzip"]
    got, gs, st = device_batches(libs[which], p1, p2, 400, gunzip="host")
    devfeed.assert_same_batches(got, files["host"](which, 400))
    assert gs == (ZERO, ZERO)


@pytest.mark.parametrize("which", LIBS)
def test_a_forced_fallback_gives_the_same_batches(libs, which, files, texts):
    """case 3: R1's member starts with stored blocks (20,000 bytes of the text as they are) followed by dynamic blocks, and chunks of 4,096 bytes
    start inside the stored part, where the text itself offers candidates.  Whatever the device leaves to zlib, the batches are the host
    feeder's"""
    t = texts[0]
    z0, z1 = zlib.compressobj(0, zlib.DEFLATED, -15), zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = z0.compress(t[:20000]) + z0.flush(zlib.Z_FULL_FLUSH) + z1.compress(t[20000:]) + z1.flush()
    data = gc.member(raw, t)
    assert gc.expected(data) == (t, 1, 0)
    blocks = gc.deflate_blocks(data)
    assert blocks[0]["btype"] == 0 and any(b["btype"] == 2 for b in blocks)
    p1 = devfeed.write(files["d"], "stored_r1.fq.gz", data)
    for kw in (dict(), dict(chunk_bytes=4096, **SMALL)):
        got, gs, st = device_batches(libs[which], p1, files["forms"]["gzip"][1], 77, **kw)
        devfeed.assert_same_batches(got, files["host"](which, 77))
        assert gs[0]["launches"] >= 1 and gs[0]["members"] == 1 and gs[0]["inflated_bytes"] == len(t)
        taken(gs[1], 1)


def _until_error(fd, target):
    out = []
    while True:
        sb = api._SuperBatch()
        n = fd.lib.arx_feeder_next(fd.h, int(target), C.byref(sb))
        if n <= 0:
            return out, n
        out.append(devfeed.snapshot(sb, n))


def _pairs(batches):
    """(name, bases of both reads, qualities of both reads) of every pair, in order"""
    out = []
    for sb in batches:
        if not sb["n_sets"]:
            continue
        lens = np.frombuffer(sb["lens"], np.int32)
        boff = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
        noff = np.frombuffer(sb["name_off"], np.int64)
        for p in range(sb["n_pairs"]):
            a, b = int(boff[2 * p]), int(boff[2 * p + 2])
            out.append((sb["names"][noff[p]:noff[p + 1]], sb["bases"][a:b], sb["quals"][a:b]))
    return out


def _set_sizes(batches):
    return [int(n) for sb in batches if sb["n_sets"] for n in np.diff(np.frombuffer(sb["set_pair_off"], np.int64))]


@pytest.mark.parametrize("which", LIBS)
@pytest.mark.parametrize("damage", ["body", "crc"])
def test_damage_ends_the_input_like_a_read_error(libs, which, damage, files, texts):
    """case 4: a byte flipped in the middle of R1's DEFLATE body, or R1's CRC-32 in the trailer.  Super-batches arrive whose sets are the
    leading sets of the undamaged input as far as the text in front of the damage reaches (zlib on the bytes in front of the flip says how
    far; behind it a decoder may go on for a while with other bytes), then arx_feeder_next returns < 0 and stays there"""
    lib = libs[which]
    z = bytearray(open(files["forms"]["gzip"][0], "rb").read())
    at = len(z) // 2 if damage == "body" else len(z) - 8
    z[at] ^= 0x5A
    intact = zlib.decompressobj(31).decompress(bytes(z[:at]))
    assert texts[0].startswith(intact) and (len(intact) > 50000 if damage == "body" else intact == texts[0])
    n_intact = intact.count(b"\n") // 4                          # pairs whose R1 record lies in front of the damage
    p1 = devfeed.write(files["d"], "damaged_%s_r1.fq.gz" % damage, bytes(z))
    want = files["host"](which, 77)
    want_pairs, want_sizes = _pairs(want), _set_sizes(want)
    for kw in (dict(), dict(chunk_bytes=4096, **SMALL)):
        fd = open_feeder(lib, p1, files["forms"]["gzip"][1], **kw)
        got, rc = _until_error(fd, 77)
        assert rc < 0 and fd.lib.arx_feeder_next(fd.h, 77, C.byref(api._SuperBatch())) < 0
        gs = fd.gunzip_stats()
        fd.close()
        assert gs[0]["launches"] >= 1
        got_pairs, got_sizes = _pairs(got), _set_sizes(got)
        if damage == "crc":
            # the whole text is intact and had entered the parse when the trailer was read: every super-batch is the host feeder's on the
            # undamaged input, except that the last set, which the error ends, is not flagged unique (device_feeder.h: next())
            assert len(got) == len(want) - 1
            for k, (a, b) in enumerate(zip(got, want)):
                assert a.keys() == b.keys()
                for key in a:
                    if k == len(got) - 1 and key in ("unique", "do_rfa"):
                        assert a[key][:-1] == b[key][:-1] and a[key][-1] == 0, key
                    else:
                        assert a[key] == b[key], (k, key)
            continue
        if kw:
            assert len(got) >= 2 and len(got_pairs) >= 77        # the launches in front of the damage were delivered before it was met
        k = min(len(got_pairs), n_intact)
        assert got_pairs[:k] == want_pairs[:k]
        whole, n = 0, 0                                          # the sets that end in front of the damage are the undamaged input's sets
        while whole < len(got_sizes) and n + got_sizes[whole] <= k:
            n += got_sizes[whole]
            whole += 1
        assert got_sizes[:max(whole - 1, 0)] == want_sizes[:max(whole - 1, 0)]


@pytest.mark.parametrize("which", LIBS)
def test_flags_and_refusals(libs, which, files):
    """case 5"""
    p1, p2 = files["forms"]["gzip"]
    ref = _ref(libs[which])
    msg = C.create_string_buffer(256)
    for flags in (8, 9):
        h = C.c_void_p()
        assert ref.lib.arx_feeder_open_device_ex(ref.h, p1.encode(), p2.encode(), 0, 1, flags, C.byref(h), msg, 256) == 0 and h.value
        ref.lib.arx_feeder_close(h)
    for flags in (2, 4, 16, -1):
        h = C.c_void_p()
        assert ref.lib.arx_feeder_open_device_ex(ref.h, p1.encode(), p2.encode(), 0, 1, flags, C.byref(h), msg, 256) == ARX_E_ARG and not h.value
        assert b"flag" in msg.value
    with pytest.raises(ValueError):
        api.Feeder(p1, p2, lib_path=libs[which], gunzip="device")            # the host feeder has no device inflate
    fd = api.Feeder(files["plain"][0], files["plain"][1], lib_path=libs[which])
    st = (C.c_int64 * (2 * len(api.GUNZIP_STATS)))()
    assert fd.lib.arx_feeder_gunzip_stats(fd.h, st) == ARX_E_ARG
    fd.close()
    for sw in (dict(gz_chunk=32), dict(gz_chunk=4096, gz_slab=4096), dict(gz_slab=1 << 28)):     # sizes outside arx_selftest_gunzip's bounds
        with pytest.raises(api.ArachneError):
            open_feeder(libs[which], p1, p2, **sw)


@pytest.mark.parametrize("which", LIBS)
def test_device_reads_are_those_of_the_plain_input(libs, which, files):
    """case 6: arx_feeder_device_reads after every super-batch, copied home: the same arrays from the gzip pair as from the plain pair"""
    lib = libs[which]

    def reads(fd, sb, snap):
        db, dl, nb = fd.device_reads()
        assert nb == len(snap["bases"])
        dev = (devfeed.copy_home(lib, db, nb), devfeed.copy_home(lib, dl, 8 * snap["n_pairs"]))
        assert dev == (snap["bases"], snap["lens"])
        seen.append(dev)

    both = []
    for paths, kw in ((files["plain"], dict(gunzip="host")), (files["forms"]["gzip"], dict(chunk_bytes=50000, **SMALL))):
        seen = []
        fd = open_feeder(lib, paths[0], paths[1], **kw)
        devfeed.feed_all(fd, 400, each=reads)
        fd.close()
        both.append(seen)
    assert len(both[0]) >= 3 and both[0] == both[1]

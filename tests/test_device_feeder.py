"""The device FASTQ feeder (arx_feeder_open_device: csrc/dev_fastq.h, device_feeder.h) against the plain-Python restatement of the reference's
reader (oracle/fastq_reader.py) and, byte for byte, against the host feeder (arx_feeder_open) -- never against its own output.  Every test
exists twice: on the host test double, where the same functors run under a sequential runtime, and on the product library (-m gpu).

Set sizes and flags are hand-derived from reader.go:209-300 as in tests/test_feeder.py; the conditions a test needs of its input (where
chunks end, which files are damaged how) are computed from the file texts and the generator, not from a feeder."""
import ctypes as C
import os
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

import devfeed
from devfeed import SIM
from arachne_amd import api, e2e, synth

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
    """a context of the library: the device feeder parses on its GPU (any index will do)"""
    if lib_path not in _REFS:
        d = tempfile.mkdtemp(prefix="arx_dfeed_ref_")
        fa = os.path.join(d, "g.fa")
        synth.make_genome(3, [20000, 6000]).write_fasta(fa)
        api.index_build(fa, fa, lib_path=lib_path)
        _REFS[lib_path] = api.Reference(fa, lib_path=lib_path)
    return _REFS[lib_path]


def _device_batches(lib_path, p1, p2, target, chunk_bytes=0, depth=1, parse_chunks=None, each=None):
    """-> (snapshots of every super-batch, arx_feeder_stats)"""
    old = os.environ.pop("ARX_FEEDER_PARSE_CHUNKS", None)
    if parse_chunks:
        os.environ["ARX_FEEDER_PARSE_CHUNKS"] = str(parse_chunks)
    try:
        fd = api.Feeder(p1, p2, device=_ref(lib_path), chunk_bytes=chunk_bytes, depth=depth)
    finally:
        os.environ.pop("ARX_FEEDER_PARSE_CHUNKS", None)
        if old is not None:
            os.environ["ARX_FEEDER_PARSE_CHUNKS"] = old
    out = devfeed.feed_all(fd, target, each)
    st = fd.stats()
    fd.close()
    return out, st


def _host_batches(lib_path, p1, p2, target):
    fd = api.Feeder(p1, p2, lib_path=lib_path)
    out = devfeed.feed_all(fd, target)
    fd.close()
    return out


def _flat(batches, key):
    return [int(x) for sb in batches if sb["n_sets"] for x in (np.diff(np.frombuffer(sb[key], np.int64)) if key == "set_pair_off" else sb[key])]


RULES = [("A-1", 3), ("B-1", 5), ("C", 7), ("D-1", 30450), ("E-1", 1), (None, 2), ("F-1", 6)]


def _rules_texts():
    t1, t2 = devfeed.fastq(RULES)
    return t1[:-1], t2[:-1]                     # no newline at the end of the files: the 6th F-1 record is cut off


@pytest.mark.parametrize("which", LIBS)
@pytest.mark.parametrize("target", [10, 1000, 10**6])
def test_barcode_set_rules(libs, which, target):
    """The input of test_feeder.test_barcode_set_rules: sizes and flags by hand (see there), every array against the restatement and byte
    for byte against the host feeder."""
    lib = libs[which]
    t1, t2 = _rules_texts()
    d = tempfile.mkdtemp(prefix="arx_dfeed_")
    p1, p2 = devfeed.write(d, "r1.fq", t1), devfeed.write(d, "r2.fq", t2)
    got, st = _device_batches(lib, p1, p2, target)
    assert _flat(got, "set_pair_off") == [3, 5, 7, 30000, 201, 201, 48, 1, 2, 5]
    assert _flat(got, "unique") == [1, 1, 1, 0, 0, 0, 1, 1, 1, 1]
    assert _flat(got, "do_rfa") == [0, 1, 0, 0, 0, 0, 1, 0, 0, 1]
    if target == 1000:
        assert [sb["n_sets"] for sb in got] == [4, 6, 0]                      # whole sets until >= 1000 pairs
    devfeed.check_against_restatement(got, t1, t2)
    devfeed.assert_same_batches(got, _host_batches(lib, p1, p2, target))
    assert st["fallback_chunks"] == 0 and st["records"] == 30473 and st["bad_lines"] == 0


@pytest.mark.parametrize("which", LIBS)
@pytest.mark.parametrize("target", [10, 1000, 10**6])
def test_gzip_bad_lines_and_header_forms(libs, which, target):
    """The input of test_feeder.test_gzip_bad_lines_and_header_forms: gzip, a stray line, BX last on the line, BX followed by nothing,
    several BX tags, VX:i:2, a header of one field."""
    lib = libs[which]
    r1 = ("@a/1 BX:Z:X-1\nACGT\n+\nIIII\n" "stray\n" "@b/1\tVX:i:1\tBX:Z:X-1\tBX:Z:Y-1\nacgn\n+\nIIII\n" "@c/1 BX:Z: VX:i:1\nAC\n+\nII\n"
          "@d/1\nA\n+\nI\n" "@e/1 BX:Z:Z-1 VX:i:2\nA\n+\nI\n")
    r2 = ("@a/2 BX:Z:X-1\nTTTT\n+\nJJJJ\n" "stray\n" "@b/2\nGGGG\n+\nJJJJ\n" "@c/2\nGG\n+\nJJ\n" "@d/2\nG\n+\nJ\n" "@e/2\nG\n+\nJ\n")
    d = tempfile.mkdtemp(prefix="arx_dfeed_")
    p1, p2 = devfeed.write(d, "r1.fq.gz", r1, gz=True), devfeed.write(d, "r2.fq.gz", r2, gz=True)
    got, st = _device_batches(lib, p1, p2, target)
    sets, bad = devfeed.check_against_restatement(got, r1, r2)
    assert [len(s[0]) for s in sets] == [2, 2, 1] and bad == 1
    assert _flat(got, "set_pair_off") == [2, 2, 1] and got[-1]["bad_lines"] == 1
    assert b"".join(sb["names"] for sb in got[:-1]) == b"abe" and b"".join(sb["barcodes"] for sb in got[:-1]) == b"X-1Z-1"
    assert b"".join(sb["rgs"] for sb in got[:-1]) == b"BX:Z:X-1BX:Z:Y-1VX:i:1VX:i:2"
    assert [int(x) for sb in got[:-1] for x in sb["valid"]] == [0, 1, 0, 0, 0]
    devfeed.assert_same_batches(got, _host_batches(lib, p1, p2, target))
    assert st["fallback_chunks"] == 0 and st["bad_lines"] == 1


@pytest.mark.parametrize("which", LIBS)
def test_counting_rule_edges(libs, which):
    """Runs of exactly 30,000, 30,001, 30,201 and 30,202 records, the first barcode again after the others, and the end of the input directly
    after a run that ended on the 30,000 cap.  By hand from reader.go:209-300: a cap leaves no record pending, so the set after it starts
    fresh; it continues the last barcode, so it breaks off at its 201st record (not unique) unless the barcode changes first (unique);
    a run that ends exactly at a cap or at the 201st record is followed by a fresh set of the next barcode; A-1 again is a run of its own
    (4 records: unique, too small for RFA); after E-1's 30,000 the reader finds the end of the input with no record in hand: no set."""
    lib = libs[which]
    groups = [("A-1", 30000), ("B-1", 30001), ("C-1", 30201), ("D-1", 30202), ("A-1", 4), ("E-1", 30000)]
    t1, t2 = devfeed.fastq_long_runs(groups)
    # a stray line directly behind a set that ends on the 30,000 cap (A-1) and behind one that ends on the 201 cap (C-1): the host feeder has
    # not read past such a set when it stops there, so the super-batch that ends with it does not count the line yet, the next one does
    cuts = [4 * 30000, 4 * (30000 + 30001 + 30201)]
    l1, l2 = t1.split("\n"), t2.split("\n")
    for c in reversed(cuts):
        l1.insert(c, "stray one"); l2.insert(c, "stray two")
    t1, t2 = "\n".join(l1), "\n".join(l2)
    d = tempfile.mkdtemp(prefix="arx_dfeed_")
    p1, p2 = devfeed.write(d, "r1.fq", t1), devfeed.write(d, "r2.fq", t2)
    for target in (10, 10**6):
        got, st = _device_batches(lib, p1, p2, target, chunk_bytes=1 << 20)
        assert _flat(got, "set_pair_off") == [30000, 30000, 1, 30000, 201, 30000, 201, 1, 4, 30000]
        assert _flat(got, "unique") == [0, 0, 1, 0, 0, 0, 0, 1, 1, 0]
        assert _flat(got, "do_rfa") == [0] * 10
        devfeed.assert_same_batches(got, _host_batches(lib, p1, p2, target))
        assert st["fallback_chunks"] == 0 and st["runs"] == 6 and st["bad_lines"] == 2
        if target == 10:              # super-batches [30000] [30000] [1, 30000] [201] [30000] [201] [1, 4, 30000] and the end: all but the last end on a cap
            assert [sb["bad_lines"] for sb in got] == [0, 1, 1, 1, 2, 2, 2, 2]
    devfeed.check_against_restatement(got, t1, t2)


def _crc(snap):
    return {k: zlib.crc32(x) if isinstance(x, bytes) else x for k, x in snap.items()}


def _line_of(text, positions):
    """index of the line that holds each byte position"""
    nl = np.flatnonzero(np.frombuffer(text.encode("latin-1"), np.uint8) == 10)
    return np.searchsorted(nl, positions, side="left")


CHUNK_CASES = [(4096, None, None), (4096, None, 1), (65536, None, None), (0, None, None), (64, 200, None), (64, 200, 1)]


@pytest.mark.parametrize("which", LIBS)
@pytest.mark.parametrize("chunk,first,parse_chunks", CHUNK_CASES)
def test_chunk_boundaries(libs, which, chunk, first, parse_chunks):
    """The 30,473-record input with chunk_bytes 4096, 65536 and the default, and its first 200 records with chunk_bytes 64 (half a
    record); 4096 and 64 also with every chunk a parse of its own, so that every chunk end the conditions count is a cut the parser sees (the
    30,000 and 201 caps then fall between parses as well).  Chunk k of a file is bytes [k * chunk, (k + 1) * chunk) of its text: where
    the chunks end is computed here from the texts."""
    lib = libs[which]
    t1, t2 = _rules_texts()
    if first:
        t1, t2 = ("".join(y + "\n" for y in x.split("\n")[:4 * first]) for x in (t1, t2))
    size = chunk or devfeed.DEFAULT_CHUNK
    n1, n2 = -(-len(t1) // size), -(-len(t2) // size)
    if chunk == 4096:
        # a chunk ends inside a line if its last byte and the next chunk's first byte lie in the same line
        cut1, cut2 = np.arange(1, n1) * size, np.arange(1, n2) * size
        l1, l2 = _line_of(t1, cut1 - 1), _line_of(t2, cut2 - 1)
        in1, in2 = l1 == _line_of(t1, cut1), l2 == _line_of(t2, cut2)
        head1, qual1, head2, qual2 = (int((i & (l % 4 == k)).sum()) for i, l in ((in1, l1), (in2, l2)) for k in (0, 3))
        print(f"R1: {n1} chunks, {head1} end inside a header, {qual1} inside a quality line; R2: {n2}, {head2}, {qual2}")
        assert min(head1, qual1, head2, qual2) >= 100
        a, b = t1.index("@read15/1"), t1.index("@read30465/1")                         # the D-1 run: records 15 .. 30464
        run_chunks = (b - 1) // size - a // size + 1
        print(f"the 30,450-record run spans {run_chunks} chunks of R1")
        assert run_chunks >= 500
        m = min(len(l1), len(l2))
        differ = (l1[:m] != l2[:m]).mean()
        print(f"chunk ends of R1 and R2 in different lines: {differ:.3f} of {m}")
        assert differ >= 0.9
    if chunk == 64:
        heads = np.array([m for m in range(len(t1)) if t1.startswith("@read", m) and (m == 0 or t1[m - 1] == "\n")])
        assert len(heads) == first and (np.diff(heads) > 64).all()                          # every record straddles chunks
    d = tempfile.mkdtemp(prefix="arx_dfeed_")
    p1, p2 = devfeed.write(d, "r1.fq", t1), devfeed.write(d, "r2.fq", t2)
    got, st = _device_batches(lib, p1, p2, 1000, chunk_bytes=chunk, parse_chunks=parse_chunks)
    assert st["chunks"] == n1 + n2                  # the forced size really applied
    assert st["bytes"] == len(t1) + len(t2) and st["fallback_chunks"] == 0
    devfeed.check_against_restatement(got, t1, t2)
    devfeed.assert_same_batches(got, _host_batches(lib, p1, p2, 1000))


N_SEEDS = 300


@pytest.mark.parametrize("which", LIBS)
def test_damaged_input_seeded(libs, which):
    """Seeded small file pairs with damaged records (devfeed.damaged_pair): equal to the restatement on every file and byte for byte to the
    host feeder, with chunk_bytes 64 (also with every chunk a parse of its own) and the default.  The conditions are asserted from the generator,
    the restatement's count of skipped lines and an independent walk over the lines, so that the test cannot pass on tame files."""
    lib = libs[which]
    d = tempfile.mkdtemp(prefix="arx_dfeed_")
    n_bad = n_at = n_unequal = 0
    for seed in range(N_SEEDS):
        t1, t2, info = devfeed.damaged_pair(seed)
        p1, p2 = devfeed.write(d, f"r1_{seed}.fq", t1), devfeed.write(d, f"r2_{seed}.fq", t2)
        want = _host_batches(lib, p1, p2, 7)
        sets, bad = devfeed.check_against_restatement(want, t1, t2)
        heads, skipped = devfeed.walk(t1, t2)
        assert len(skipped) == bad
        n_bad += bad > 0
        n_at += bool(set(heads) & set(info["at_qual"]))         # a quality line that starts with '@' where the search looked: read as a header
        n_unequal += info["unequal"]
        for chunk, parse_chunks in ((64, None), (64, 1), (0, None)):
            if which == "gpu" and parse_chunks and seed % 4:
                continue                                         # a parse per 64 bytes: every fourth file is enough on the GPU
            got, st = _device_batches(lib, p1, p2, 7, chunk_bytes=chunk, parse_chunks=parse_chunks)
            devfeed.check_against_restatement(got, t1, t2)
            devfeed.assert_same_batches(got, want)
            assert st["bad_lines"] == bad and st["fallback_chunks"] == 0, seed
    print(f"{N_SEEDS} files: {n_bad} with skipped lines, {n_at} with an '@' quality line read as a header, {n_unequal} with unequal line counts")
    assert n_bad >= 50 and n_at >= 50 and n_unequal >= 30


@pytest.mark.parametrize("which", LIBS)
def test_beyond_the_restatement(libs, which):
    """Hand-written files the restatement does not accept (the reference panics on them), compared with the host feeder only: a header
    that is '@' alone, headers of white space, bytes >= 0x80 in every kind of line, NUL bytes, empty files, a file of one unterminated line."""
    lib = libs[which]
    cases = [
        (b"@\nACGT\n+\nIIII\n@ \t\nAC\n+\nII\n@x/1 BX:Z:A-1\nA\n+\nI\n", b"@\nTTTT\n+\nJJJJ\n@\nGG\n+\nJJ\n@x/2\nC\n+\nJ\n"),
        (b"@r\xe9ad/1 BX:Z:\xff\x80-1 VX:i:1\nAC\xc7T\n+\n\x80\x81\x82\x83\n@q/1\xa0BX:Z:B-1\nA\x00C\n+\nI\x00I\n", b"@a\nTT\xffT\n+\nJJJJ\n@b\nG\x00G\n+\n\xfe\xfe\xfe\n"),
        (b"", b""),
        (b"@a/1 BX:Z:A-1", b"@a/2"),
        (b"\n\n\n@a/1 BX:Z:A-1\nA\n+\nI\n\n", b"\n\n\n@a/2\nC\n+\nJ\n\n"),
    ]
    d = tempfile.mkdtemp(prefix="arx_dfeed_")
    for k, (b1, b2) in enumerate(cases):
        p1, p2 = devfeed.write(d, f"r1_{k}.fq", b1), devfeed.write(d, f"r2_{k}.fq", b2)
        want = _host_batches(lib, p1, p2, 10)
        for chunk, parse_chunks in ((64, None), (16, 1), (0, None)):
            got, st = _device_batches(lib, p1, p2, 10, chunk_bytes=chunk, parse_chunks=parse_chunks)
            devfeed.assert_same_batches(got, want)
    with pytest.raises(api.ArachneError, match="cannot open"):
        api.Feeder("/nonexistent/r1.fq", "/nonexistent/r2.fq", device=_ref(lib))


def _placement_files(lib_path, n_bc, ppb, gz):
    g = synth.make_genome(5, [300000, 100000])
    rs = synth.make_reads(6, g, n_bc, ppb)
    d = tempfile.mkdtemp(prefix="arx_dfeed_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    g.write_alt(fa + ".alt")
    api.index_build(fa, fa, lib_path=lib_path)
    po = rs.pair_offsets()
    r1, r2 = [], []
    for b in range(len(po) - 1):
        for p in range(int(po[b]), int(po[b + 1])):
            for side, out in ((0, r1), (1, r2)):
                s = "".join("ACGTN"[x] for x in rs.seqs[2 * p + side][:rs.lens[2 * p + side]])
                out.append(f"@p{p}/{side + 1} BX:Z:{rs.barcodes[b]} VX:i:1\n{s}\n+\n{'I' * len(s)}\n")
    ext = ".fq.gz" if gz else ".fq"
    return fa, devfeed.write(d, "r1" + ext, "".join(r1), gz=gz), devfeed.write(d, "r2" + ext, "".join(r2), gz=gz), rs


@pytest.mark.parametrize("which,n_bc,ppb,gz,target", [pytest.param("sim", 4, 60, False, 100, id="hostsim"),
                                                      pytest.param("gpu", 12, 400, True, 3000, id="gpu", marks=pytest.mark.gpu)])
def test_device_arrays(libs, which, n_bc, ppb, gz, target):
    """arx_feeder_device_reads copied home equals the host arrays, and a batch filled by arx_batch_reset_device from them gives the
    regions, alignments and placements of a batch created from the host feeder's arrays (two super-batches at least)."""
    lib = libs[which]
    fa, p1, p2, rs = _placement_files(lib, n_bc, ppb, gz)
    ref = api.Reference(fa, lib_path=lib)
    try:
        fd_dev, fd_host = api.Feeder(p1, p2, device=ref, chunk_bytes=65536, depth=2), api.Feeder(p1, p2, lib_path=lib)
        handle = None
        n_batches = 0
        while True:
            hb = fd_host.next(target)
            nx = fd_dev.next_raw(target)
            assert (hb is None) == (nx is None)
            if hb is None:
                break
            n_batches += 1
            sb, v = nx
            d_bases, d_lens, n_bases = fd_dev.device_reads()
            P = int(v["n_pairs"])
            assert P == hb["n_pairs"] and n_bases == len(hb["bases"])
            assert devfeed.copy_home(lib, d_lens, 8 * P) == hb["lens"].tobytes() == v["lens"].tobytes()
            assert devfeed.copy_home(lib, d_bases, n_bases) == hb["bases"].tobytes() == v["bases"].tobytes()
            a = ref.batch(hb["bases"], hb["lens"]).run()
            if handle is None:
                handle = ref.batch(np.zeros(2, np.uint8), np.ones(2, np.int32))
            handle.reset_device(2 * P, n_bases, d_bases, d_lens).run()
            fa_, fb_ = a.fetch(), handle.fetch()
            assert fa_.keys() == fb_.keys() and len(fa_["regs"]) > 0
            for key in ("reg_off", "regs", "alns", "cigars"):
                assert fa_[key].tobytes() == fb_[key].tobytes(), key
            assert fa_["counts"] == fb_["counts"]
            ca, cb = a.rfa(hb["set_pair_off"], hb["do_rfa"]), handle.rfa(v["set_pair_off"], v["do_rfa"])
            assert (ca["cand_off"] == cb["cand_off"]).all() and ca["cands"].tobytes() == cb["cands"].tobytes() and len(ca["cands"]) > 0
            a.free()
        assert n_batches >= 2 and fd_dev.stats()["fallback_chunks"] == 0 and fd_dev.stats()["records"] == rs.n_pairs
        handle.free()
        fd_dev.close()
        fd_host.close()
    finally:
        ref.close()


@pytest.mark.parametrize("which", LIBS)
def test_depth_keeps_super_batches_valid(libs, which):
    """depth = 3: the arrays of super-batch k, host and device, still hold after calls k + 1 and k + 2 (checksums taken when it was
    delivered and again after the two calls); depth = 1: the plain contract, every super-batch whole while it is the last one."""
    lib = libs[which]
    t1, t2 = devfeed.fastq([(f"B{k}-1", 40 + 7 * (k % 5)) for k in range(30)], seed=3)
    d = tempfile.mkdtemp(prefix="arx_dfeed_")
    p1, p2 = devfeed.write(d, "r1.fq", t1), devfeed.write(d, "r2.fq", t2)
    want = _host_batches(lib, p1, p2, 150)
    assert len(want) >= 8

    def sums(fd, sb, n):
        snap = devfeed.snapshot(sb, n)
        db, dl, nb = fd.device_reads()
        assert nb == len(snap["bases"])
        dev = (devfeed.copy_home(lib, db, nb), devfeed.copy_home(lib, dl, 8 * snap["n_pairs"]))
        assert dev == (snap["bases"], snap["lens"])
        return _crc(snap), zlib.crc32(dev[0]), zlib.crc32(dev[1]), (db, dl, nb, snap["n_pairs"])

    for depth in (3, 1):
        fd = api.Feeder(p1, p2, device=_ref(lib), chunk_bytes=4096, depth=depth)
        held = []                                  # (struct, n_sets, checksums) of the last `depth` super-batches
        k = 0
        while True:
            sb = api._SuperBatch()
            n = fd.lib.arx_feeder_next(fd.h, 150, C.byref(sb))
            if n == 0:
                break
            now = sums(fd, sb, n)
            assert now[0] == _crc(want[k])
            held.append((sb, n, now))
            held = held[-depth:]
            for osb, on, (osnap, ob, ol, (db, dl, nb, P)) in held[:-1]:        # delivered up to depth - 1 calls ago
                assert _crc(devfeed.snapshot(osb, on)) == osnap
                assert zlib.crc32(devfeed.copy_home(lib, db, nb)) == ob and zlib.crc32(devfeed.copy_home(lib, dl, 8 * P)) == ol
            k += 1
        assert k == len(want) - 1 and fd.stats()["fallback_chunks"] == 0
        fd.close()


@pytest.mark.parametrize("which,n_bc,ppb", [pytest.param("sim", 6, 60, id="hostsim"), pytest.param("gpu", 24, 500, id="gpu", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("layout", ["workers", "reference"])
def test_end_to_end_one_pair(libs, which, n_bc, ppb, layout):
    """e2e.run(feeder="device", workers=3) on ONE file pair against e2e.run with the host feeder on the same pair: the same multiset of records
    per output file, read back with an independent BAM reader (the order of super-batches across workers is free; with layout="workers" the
    three workers' files together hold what the host run's one file holds)."""
    lib = libs[which]
    g = synth.make_genome(15, [400000, 150000])
    rs = synth.make_reads(16, g, n_bc, ppb, invalid_frac=0.25)
    d = tempfile.mkdtemp(prefix="arx_dfeed_e2e_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    api.index_build(fa, fa, lib_path=lib)
    f1, f2 = os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq")
    synth.write_fastq_fast(rs, f1, f2)
    ref = api.Reference(fa, lib_path=lib)
    try:
        kw = dict(pairs_per_batch=max(50, rs.n_pairs // 7), bam_threads=2, rec_threads=3, lib_path=lib, layout=layout, chunk=100000)
        host = e2e.run(ref, [(f1, f2)], os.path.join(d, "host"), **kw)
        dev = e2e.run(ref, [(f1, f2)], os.path.join(d, "dev"), feeder="device", workers=3, chunk_bytes=65536, **kw)
        assert dev["pairs"] == host["pairs"] == rs.n_pairs and dev["records"] == host["records"] and dev["batches"] == host["batches"] >= 5
        assert dev["feeder"]["fallback_chunks"] == 0 and dev["feeder"]["records"] == rs.n_pairs
        if layout == "workers":
            a = sorted(devfeed.bam_records(os.path.join(d, "host.0.bam")))
            b = sorted(r for k in range(3) for r in devfeed.bam_records(os.path.join(d, f"dev.{k}.bam")))
            assert len(a) == 2 * rs.n_pairs and a == b
        else:
            assert host["files"] == dev["files"] and len(host["files"]) >= 4
            total = 0
            for f in host["files"]:
                a, b = sorted(devfeed.bam_records(os.path.join(d, "host", f))), sorted(devfeed.bam_records(os.path.join(d, "dev", f)))
                assert a == b, f
                total += len(a)
            assert total >= 4 * rs.n_pairs           # every record twice: bc_sorted_bam.bam and its bucket
    finally:
        ref.close()


@pytest.mark.parametrize("which,n_bc,ppb", [pytest.param("sim", 16, 30, id="hostsim"), pytest.param("gpu", 16, 200, id="gpu", marks=pytest.mark.gpu)])
def test_end_to_end_one_slow_worker(libs, which, n_bc, ppb, monkeypatch):
    """One worker is held up in its first super-batch (arx_batch_rfa sleeps) while the other two go on taking super-batches: the feeder's
    arrays of that first super-batch must still be whole when its records are built -- the producer may run at most depth - 1 calls ahead of
    the OLDEST super-batch in use, however many newer ones are done.  Same records as the host-feeder run, and the held-up worker must have
    seen the others pass it (or the producer wait for it)."""
    import threading
    import time
    lib = libs[which]
    g = synth.make_genome(15, [400000, 150000])
    rs = synth.make_reads(16, g, n_bc, ppb, invalid_frac=0.25)
    d = tempfile.mkdtemp(prefix="arx_dfeed_slow_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    api.index_build(fa, fa, lib_path=lib)
    f1, f2 = os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq")
    synth.write_fastq_fast(rs, f1, f2)
    ref = api.Reference(fa, lib_path=lib)
    try:
        kw = dict(pairs_per_batch=max(10, rs.n_pairs // 24), bam_threads=2, rec_threads=2, lib_path=lib)
        host = e2e.run(ref, [(f1, f2)], os.path.join(d, "host"), **kw)
        assert host["batches"] >= 14                      # twice the feeder's slots at workers = 3 (depth 5: seven)
        real_rfa, lock, seen = api.Batch.rfa, threading.Lock(), dict(calls=0, at_wake=0)

        def slow_rfa(self, *a, **k):
            with lock:
                seen["calls"] += 1
                first = seen["calls"] == 1
            if first:
                t = time.time()
                while seen["calls"] < 12 and time.time() - t < 2.0:
                    time.sleep(0.01)
                seen["at_wake"] = seen["calls"]
            return real_rfa(self, *a, **k)
        monkeypatch.setattr(api.Batch, "rfa", slow_rfa)
        dev = e2e.run(ref, [(f1, f2)], os.path.join(d, "dev"), feeder="device", workers=3, chunk_bytes=65536, **kw)
        monkeypatch.undo()
        print(f"the held-up worker woke after {seen['at_wake']} of {dev['batches']} super-batches had reached arx_batch_rfa")
        assert dev["pairs"] == rs.n_pairs and dev["batches"] == host["batches"] and seen["at_wake"] >= 4
        a = sorted(devfeed.bam_records(os.path.join(d, "host.0.bam")))
        b = sorted(r for k in range(3) for r in devfeed.bam_records(os.path.join(d, f"dev.{k}.bam")))
        assert len(a) == 2 * rs.n_pairs and a == b
    finally:
        ref.close()

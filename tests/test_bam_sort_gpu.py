"""The coordinate sort of a BAM file on the GPU (arx_bam_sort_append, arx_selftest_bam_sort, arx_bam_open_ex; arachne_amd/csrc/dev_bamsort.h,
hip_bamsort.h).  1. the cases of sortcases.py -- the ones tests/test_bam_sort_sim.py runs through the host program -- through the kernels, held
to Python's stable sorted(); 2. files: written by the host writer, sorted into a host and into a device writer; 3. end to end: the reference
layout's buckets of the crafted pairs into one BAM, by e2e.finalize with both sinks."""
import os
import struct
import tempfile

import numpy as np
import pytest

import bgzfio
import reccases as rc
import recfullcases as fc
import sortcases as sc
import test_bam_reference_layout as trl
from arachne_amd import api, e2e, synth

pytestmark = pytest.mark.gpu


# ---- 1. the kernels on plain record bytes
@pytest.mark.parametrize("seg", sc.SEGS)
def test_cases_through_the_kernels(seg):
    for name, case in sc.cases().items():
        r = api.selftest_bam_sort(case.stream, case.n_ref, seg)
        st = r["stats"]
        print(name, seg, st)
        assert r["rc"] == 0 and r["n_records"] == case.n == st["records"], name
        assert r["out"] == case.out and r["guard"] == b"\xa5" * 8, name
        assert r["rec_off"][:case.n + 1].tolist() == case.rec_off.tolist() and (r["rec_off"][case.n + 1:] == -1).all(), name
        segments = -(-len(case.stream) // seg)
        assert st["segments"] == segments and st["guess_right"] + st["repaired"] == max(segments - 1, 0) and st["rounds"] <= segments, name
        if name == "decoy":
            assert st["repaired"] >= 1                      # the fake chain was the guess, and was walked again
        c = api.selftest_bam_sort(case.stream, case.n_ref, seg, mode="copy")
        assert c["rc"] == 0 and c["out"] == case.stream and c["rec_off"][:case.n + 1].tolist() == case.in_off.tolist(), name


@pytest.mark.parametrize("seg", sc.SEGS)
def test_broken_chains_are_an_error_and_nothing_is_written(seg):
    for name, s in sc.broken().items():
        for mode in ("coordinate", "copy"):
            r = api.selftest_bam_sort(s, sc.N_REF, seg, mode=mode)
            assert r["rc"] == api.ARX_E_IO, name
            assert r["out"] == b"\xa5" * len(s) and (r["rec_off"] == -1).all() and r["n_records"] == 0, name


def test_bad_arguments():
    for seg in (0, 32, 96):
        with pytest.raises(api.ArachneError) as e:
            api.selftest_bam_sort(b"", 1, seg)
        assert e.value.code == api.ARX_E_ARG


# ---- 2. files
@pytest.fixture(scope="module")
def ref():
    g = synth.make_genome(15, [400000, 150000, 3000])
    d = tempfile.mkdtemp(prefix="arx_bamsort_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    api.index_build(fa, fa)
    r = api.Reference(fa)
    r.dir = d
    yield r
    r.close()


HDR = "@PG\tID:t\n"


@pytest.fixture(scope="module")
def bucket(ref):
    """a few thousand records through the host writer: they straddle its BGZF blocks (cut every 65280 bytes) -> (path, the records)"""
    rng = np.random.default_rng(3)
    names, offs, clens, alt, l_pac = ref.contigs()
    assert len(names) == sc.N_REF
    recs = [sc.rec(int(rng.integers(-1, 3)), int(rng.integers(-1, 2000)), b"r%d" % k, l_seq=int(rng.integers(0, 200)), aux=b"NMC" + bytes([k % 7])) for k in range(4000)]
    p = os.path.join(ref.dir, "bucket.bam")
    w = api.BamWriter(p, names, clens, extra_header=HDR, threads=2, level=1)
    for a in range(0, len(recs), 700):
        w.write_encoded(b"".join(recs[a:a + 700]), len(recs[a:a + 700]))
    w.close()
    raw = open(p, "rb").read()
    blocks = bgzfio.split(raw)
    data = bgzfio.inflate(raw)
    assert len(blocks) > 8
    off = rc.header_len(data) + np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    cuts = np.cumsum([b["isize"] for b in blocks])[1:-2]                  # where the blocks behind the header's end
    starts = set(off.tolist())
    assert sum(int(c) not in starts for c in cuts) >= 5                  # ... inside records
    return p, recs


def _final(ref, path, device, coordinate=True):
    names, offs, clens, alt, l_pac = ref.contigs()
    return api.BamWriter(path, names, clens, extra_header=HDR, threads=2, level=1, device=ref if device else None, coordinate=coordinate)


def _expected_header(ref, so):
    names, offs, clens, alt, l_pac = ref.contigs()
    text = ("@HD\tVN:1.6\tSO:%s\n" % so + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in zip(names, clens)) + HDR).encode()
    refs = b"".join(struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l) for n, l in zip(names, clens))
    return b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(names)) + refs


def test_sort_into_a_host_and_a_device_writer(ref, bucket):
    path, recs = bucket
    want = _expected_header(ref, "coordinate") + b"".join(sorted(recs, key=sc.key))
    for device in (False, True):
        out = os.path.join(ref.dir, "sorted_%d.bam" % device)
        w = _final(ref, out, device)
        st = w.sort_append(ref, path)
        closed = w.close()
        print("device writer" if device else "host writer", st)
        assert st["records"] == closed["records"] == len(recs) and st["blocks"] == len(bgzfio.split(open(path, "rb").read())) and st["slabs"] == 1
        assert bgzfio.inflate(open(out, "rb").read()) == want, device


def test_copy_mode_in_slabs(ref, bucket):
    path, recs = bucket
    want = _expected_header(ref, "unknown") + b"".join(recs)
    for device in (False, True):
        out = os.path.join(ref.dir, "copied_%d.bam" % device)
        w = _final(ref, out, device, coordinate=False)
        st = w.sort_append(ref, path, mode="copy", max_bytes=200000)
        closed = w.close()
        assert st["slabs"] >= 3 and st["records"] == closed["records"] == len(recs)
        assert bgzfio.inflate(open(out, "rb").read()) == want, device


def _refused(ref, path, code, **kw):
    """sort_append of `path` is refused with `code`, and nothing was appended"""
    out = os.path.join(ref.dir, "refused.bam")
    w = _final(ref, out, False)
    with pytest.raises(api.ArachneError) as e:
        w.sort_append(ref, path, **kw)
    assert e.value.code == code, str(e.value)
    assert w.close()["records"] == 0
    assert bgzfio.inflate(open(out, "rb").read()) == _expected_header(ref, "coordinate")
    return str(e.value)


def test_what_is_refused(ref, bucket):
    path, recs = bucket
    d = ref.dir
    assert "bucket" in _refused(ref, path, api.ARX_E_TOO_LARGE, max_bytes=100000)               # sort mode holds the file whole
    names, offs, clens, alt, l_pac = ref.contigs()
    foreign = os.path.join(d, "foreign.bam")
    api.BamWriter(foreign, list(names[:2]) + ["other"], clens, extra_header=HDR, threads=1).close()
    _refused(ref, foreign, api.ARX_E_ARG)
    _refused(ref, foreign, api.ARX_E_ARG, mode="copy")
    _refused(ref, os.path.join(d, "no_such_file.bam"), api.ARX_E_IO)
    plain = os.path.join(d, "plain.bam")
    with open(plain, "wb") as f:
        f.write(b"not a BGZF file at all, but long enough to hold a header " * 4)
    _refused(ref, plain, api.ARX_E_IO)
    data = bgzfio.inflate(open(path, "rb").read())
    cut = os.path.join(d, "cut.bam")
    bgzfio.write_bgzf_file(cut, data[:-7])                                                       # the last record runs past the end
    _refused(ref, cut, api.ARX_E_IO)
    _refused(ref, cut, api.ARX_E_IO, mode="copy", max_bytes=200000)
    raw = bytearray(open(path, "rb").read())
    blocks = bgzfio.split(bytes(raw))
    raw[blocks[3]["at"] + blocks[3]["size"] - 8] ^= 0x55                                         # a CRC that does not match
    bad = os.path.join(d, "badcrc.bam")
    with open(bad, "wb") as f:
        f.write(raw)
    _refused(ref, bad, api.ARX_E_IO)
    _refused(ref, bad, api.ARX_E_IO, mode="copy", max_bytes=200000)


def test_a_header_only_file_gives_no_records(ref):
    names, offs, clens, alt, l_pac = ref.contigs()
    p = os.path.join(ref.dir, "header_only.bam")
    api.BamWriter(p, names, clens, extra_header=HDR, threads=1).close()
    for mode in ("coordinate", "copy"):
        out = os.path.join(ref.dir, "from_header_only.bam")
        w = _final(ref, out, False)
        assert w.sort_append(ref, p, mode=mode)["records"] == 0
        assert w.close()["records"] == 0
        assert bgzfio.inflate(open(out, "rb").read()) == _expected_header(ref, "coordinate")


# ---- 3. end to end: the buckets of a reference-layout run into one BAM
def test_finalize_makes_one_coordinate_sorted_bam():
    g, rs = trl._reads(5, 60)                                            # the crafted pairs of tests/test_e2e_arms.py: split records are present
    d = tempfile.mkdtemp(prefix="arx_final_")
    fa = rc.make_index(d, g, api.LIB_PATH)
    f1, f2 = os.path.join(d, "a1.fq"), os.path.join(d, "a2.fq")
    synth.write_fastq_fast(rs, f1, f2)
    ref = api.Reference(fa)
    try:
        out = os.path.join(d, "out")
        st = e2e.run(ref, [(f1, f2)], out, pairs_per_batch=70, bam_threads=2, rec_threads=3, layout="reference", chunk=fc.CHUNK, final_bam=os.path.join(d, "final_host.bam"))
        paths = fc.e2e_paths(st, "reference", out)
        names, offs, clens, alt, l_pac = ref.contigs()
        table = api.bucket_table(names, clens, fc.CHUNK)
        in_order = [r for f in table.files for r in fc.records_of(paths[f])]          # the bucket files' records, in table order
        n_main = len(fc.records_of(paths["bc_sorted_bam.bam"]))
        assert len(in_order) == n_main == st["records"] == st["final"]["records"]
        want = sorted(in_order, key=sc.key)                                           # stable: equal keys keep bucket-file order
        un = [r for r in in_order if sc.key(r)[0] == 0xFFFFFFFF]
        assert 0 < len(un) < len(in_order) and want[-len(un):] == fc.records_of(paths["ZZZ_unmapped_pos_bucketed.bam"])
        fin = e2e.finalize(ref, out, os.path.join(d, "final_device.bam"), sink="device", chunk=fc.CHUNK, bam_threads=2)
        assert fin["records"] == n_main and fin["buckets"] == st["final"]["buckets"] >= 3
        for name in ("final_host.bam", "final_device.bam"):
            data = rc.inflate(os.path.join(d, name))
            text = data[8:8 + struct.unpack_from("<i", data, 4)[0]]
            assert text.startswith(b"@HD\tVN:1.6\tSO:coordinate\n")
            got = fc.records_of(os.path.join(d, name))                                # (walks the chain: the independent reader accepts the file)
            keys = [sc.key(r) for r in got]
            assert keys == sorted(keys) and sorted(got) == sorted(in_order)           # keys never decrease; the multiset of all bucket files' records
            assert got == want, name                                                  # equal keys in bucket-file order, the unmapped last
    finally:
        ref.close()

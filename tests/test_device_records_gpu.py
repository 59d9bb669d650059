"""The records phase on the GPU (arx_batch_records, arx_bam_write_encoded, arx_bam_write_encoded_device; arachne_amd/csrc/dev_records.h,
pipeline_records.h, hip_bgzf.h): the record stream the kernels write against the EXISTING host path -- arx_recbuf_build -> arx_bam_write on a
host writer, the file inflated block by block.  Everything is byte-exact.  Host-double variant with the lifetime and argument tests:
tests/test_device_records.py."""
import os
import tempfile

import numpy as np
import pytest

import bgzfcases
import reccases as rc
import workloads
from arachne_amd import api, e2e, synth

pytestmark = pytest.mark.gpu
LIB = api.LIB_PATH


def _open(genome, prefix):
    d = tempfile.mkdtemp(prefix=prefix)
    fa = rc.make_index(d, genome, LIB)
    r = api.Reference(fa)
    r.genome, r.dir = genome, d
    return r


@pytest.fixture(scope="module")
def ref():
    r = _open(synth.make_genome(31, [300000]), "arx_recgpu_")
    yield r
    r.close()


def _identity(ref, f1, f2, not_unique=()):
    fd = api.Feeder(f1, f2, lib_path=LIB)
    sb, v = fd.next_raw(10 ** 7)
    sb, keep = rc.with_unique(sb, v, set(not_unique))
    c = rc.Case(ref, sb, v, LIB)
    for dup in (True, False):
        data = rc.host_file(os.path.join(ref.dir, f"h{int(dup)}.bam"), ref, LIB, [c.host_view(dup)])
        h = rc.header_len(data)
        n, nb = c.batch.records(sb, dup=dup)
        assert (n, nb) == (2 * int(v["n_pairs"]), len(data) - h)
        stream, off = c.batch.records_fetch()
        assert stream.tobytes() == data[h:]
        assert np.array_equal(off, rc.walk(data[h:])[0])
        p = os.path.join(ref.dir, f"e{int(dup)}.bam")
        w = rc.open_writer(p, ref, LIB)
        w.write_encoded(stream, n)
        w.close()
        assert rc.inflate(p) == data
    c.free()
    fd.close()
    return n


def test_crafted_workload(ref):
    pairs = rc.crafted_pairs(ref.genome)
    f1, f2 = os.path.join(ref.dir, "c1.fq"), os.path.join(ref.dir, "c2.fq")
    rc.write_fastq(pairs, f1, f2)
    assert _identity(ref, f1, f2, {"AAAT-1"}) == 2 * len(pairs)


def test_nasty_set():
    g = workloads.nasty_genome(3)
    r = _open(g, "arx_recgpu_nasty_")
    try:
        rs = workloads.nasty_reads(3, g)
        f1, f2 = os.path.join(r.dir, "n1.fq"), os.path.join(r.dir, "n2.fq")
        synth.write_fastq_fast(rs, f1, f2)
        assert _identity(r, f1, f2) == 2 * rs.n_pairs
    finally:
        r.close()


def test_device_stream_into_device_sink(ref):
    """36 barcodes x 800 pairs as three super-batches -- 34 barcodes (a record stream of more than 256 BGZF blocks: one compressor group and
    the start of the next), one, one -- into ONE device writer: write_encoded_device, a host write_view, write_encoded_device.  The file's
    framing is valid and it inflates to the host path's file."""
    rs = synth.make_reads(5, ref.genome, 36, 800, fast=True)
    f1, f2 = os.path.join(ref.dir, "b1.fq"), os.path.join(ref.dir, "b2.fq")
    synth.write_fastq_fast(rs, f1, f2)
    fd = api.Feeder(f1, f2, lib_path=LIB)
    ph, pd = os.path.join(ref.dir, "big_h.bam"), os.path.join(ref.dir, "big_d.bam")
    wh, wd = rc.open_writer(ph, ref, LIB), rc.open_writer(pd, ref, LIB, device=ref)
    sizes = []
    for k, target in enumerate((34 * 800, 1, 1)):
        sb, v = fd.next_raw(target)
        c = rc.Case(ref, sb, v, LIB)
        view = c.host_view(True)
        wh.write_view(view)
        if k == 1:
            wd.write_view(view)
        else:
            n, nb = c.batch.records(sb)
            ptr, vb, vn = c.batch.records_view()
            assert (vb, vn) == (nb, n) and ptr
            wd.write_encoded_device(ptr, nb, n)
            sizes.append(nb)
        c.free()
    assert fd.next_raw(1) is None
    fd.close()
    sh, sd = wh.close(), wd.close()
    assert sizes[0] > 256 * 65280, sizes
    assert (sd["records"], sd["blocks"], sd["bytes_in"]) == (sh["records"], sh["blocks"], sh["bytes_in"]) and sd["records"] == 2 * rs.n_pairs
    raw = open(pd, "rb").read()
    assert raw.endswith(bgzfcases.EOF_BLOCK) and len(raw) == sd["bytes_out"]
    blocks = bgzfcases.bgzf_blocks(raw)                        # BC field, BSIZE, CRC-32, ISIZE of every block
    want = rc.inflate(ph)
    assert b"".join(b for b, _ in blocks) == want
    # cut where the host writer cuts: the header's own block, then every 65280 bytes, the EOF block
    hl = rc.header_len(want)
    assert [len(b) for b, _ in blocks] == [hl] + [min(65280, len(want) - o) for o in range(hl, len(want), 65280)] + [0]


def test_device_stream_is_refused_by_a_host_writer(ref):
    w = rc.open_writer(os.path.join(ref.dir, "refuse.bam"), ref, LIB)
    with pytest.raises(api.ArachneError, match="only arx_bam_open_device's writers take a device stream"):
        w.write_encoded_device(1 << 20, 64, 1)
    assert api._selftest_fn(w.lib, "arx_bam_write_encoded_device")(w.h, 1 << 20, 64, 1) == -2
    w.close()


def test_end_to_end_device_records_device_sink(ref):
    rs = synth.make_reads(16, ref.genome, 20, 100, invalid_frac=0.25)
    d = tempfile.mkdtemp(prefix="e2e_", dir=ref.dir)
    f1, f2 = os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq")
    synth.write_fastq_fast(rs, f1, f2)
    out = {}
    for records, sink in (("host", "host"), ("device", "device")):
        o = os.path.join(d, f"{records}_{sink}")
        st = e2e.run(ref, [(f1, f2)], o, pairs_per_batch=700, bam_threads=2, rec_threads=3, records=records, sink=sink)
        assert st["pairs"] == rs.n_pairs and st["records"] == 2 * rs.n_pairs and st["batches"] >= 2
        out[records, sink] = rc.inflate(o + ".0.bam")
    assert out["device", "device"] == out["host", "host"]
    assert len(out["host", "host"]) > 65280
    # the device feeder in front: one producer, two workers, each with its own file; a super-batch goes to whichever worker is free, so the
    # files are compared as sets of records
    for records, sink in (("host", "host"), ("device", "device")):
        o = os.path.join(d, f"f_{records}_{sink}")
        st = e2e.run(ref, [(f1, f2)], o, pairs_per_batch=700, bam_threads=2, rec_threads=3, records=records, sink=sink, feeder="device", workers=2)
        assert st["pairs"] == rs.n_pairs and st["records"] == 2 * rs.n_pairs
        recs = []
        for f in st["files"]:
            data = rc.inflate(f)
            s = data[rc.header_len(data):]
            off = rc.walk(s)[0]
            recs += [s[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        out["f", records] = sorted(recs)
    assert out["f", "device"] == out["f", "host"] and len(out["f", "host"]) == 2 * rs.n_pairs

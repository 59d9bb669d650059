"""The full records phase on the GPU (arx_batch_records_full, arx_batch_records_buckets_fetch / _view, arx_selftest_rec_text; arachne_amd/csrc/
dev_records_full.h, pipeline_records.h): both streams the kernels write against the EXISTING host path -- arx_recbuf_build_full ->
arx_bam_write for the stream, arx_bam_write_select for every bucket, the files inflated.  Everything is byte-exact.  Host-double variant with
the coverage, lifetime and argument tests: tests/test_device_records_full.py."""
import os
import tempfile

import numpy as np
import pytest

import bgzfcases
import reccases as rc
import recfullcases as fc
import test_bam_reference_layout as trl
import workloads
from arachne_amd import api, e2e, synth

pytestmark = pytest.mark.gpu
LIB = api.LIB_PATH


def test_crafted_workload():
    d = tempfile.mkdtemp(prefix="arx_recfullgpu_")
    w = fc.World(LIB, d)
    try:
        c = fc.FullCase(w.ref, w.sb, w.v, w.table, LIB, d, "host")
        n, nb = fc.check_identity(c)
        assert n > 2 * len(w.pairs)
        c.free()
    finally:
        w.close()


def test_nasty_set():
    g = workloads.nasty_genome(3)
    d = tempfile.mkdtemp(prefix="arx_recfullgpu_nasty_")
    fa = rc.make_index(d, g, LIB)
    ref = api.Reference(fa)
    try:
        rs = workloads.nasty_reads(3, g)
        f1, f2 = os.path.join(d, "n1.fq"), os.path.join(d, "n2.fq")
        synth.write_fastq_fast(rs, f1, f2)
        names, _, clens, _, _ = ref.contigs()
        table = api.bucket_table(names, clens, 20000, lib_path=LIB)
        fd = api.Feeder(f1, f2, lib_path=LIB)
        sb, v = fd.next_raw(10 ** 7)
        c = fc.FullCase(ref, sb, v, table, LIB, d, "host")
        assert fc.check_identity(c)[0] >= 2 * rs.n_pairs
        c.free()
        fd.close()
    finally:
        ref.close()


@pytest.fixture(scope="module")
def big():
    g, rs = trl._reads(20, 200)                                     # 4000 pairs, chimeras among them
    d = tempfile.mkdtemp(prefix="arx_recfullgpu_big_")
    fa = rc.make_index(d, g, LIB)
    f1, f2 = os.path.join(d, "b1.fq"), os.path.join(d, "b2.fq")
    synth.write_fastq_fast(rs, f1, f2)
    ref = api.Reference(fa)
    yield dict(rs=rs, d=d, files=(f1, f2), ref=ref)
    ref.close()


def test_both_streams_into_device_writers(big):
    """one super-batch of 4000 pairs: the stream and every bucket's slice of the grouped stream from device memory into DEVICE writers"""
    ref, d = big["ref"], big["d"]
    names, _, clens, _, _ = ref.contigs()
    table = api.bucket_table(names, clens, fc.CHUNK, lib_path=LIB)
    fd = api.Feeder(*big["files"], lib_path=LIB)
    sb, v = fd.next_raw(10 ** 7)
    c = fc.FullCase(ref, sb, v, table, LIB, d, "host")
    sizes = [len(b) for b in c.bucket_body]
    assert max(sizes) > 65280 and 0 < min(s for s in sizes if s) < 65280, sizes     # from the host path: slices longer and shorter than a BGZF block
    n, nb = fc.check_identity(c)
    assert n > 2 * big["rs"].n_pairs and n > 16 * 256                                  # many blocks of the grouping
    ptr, vb, vn = c.batch.records_view()
    gptr, bo, ro = c.batch.records_buckets_view()
    assert (vb, vn) == (nb, n) and ptr and gptr
    paths = [os.path.join(d, "dev_%d.bam" % k) for k in range(len(table.files) + 1)]
    ws = [rc.open_writer(p, ref, LIB, device=ref) for p in paths]
    ws[0].write_encoded_device(ptr, nb, n)
    for f in range(len(table.files)):
        if ro[f + 1] > ro[f]:
            ws[f + 1].write_encoded_device(gptr + int(bo[f]), int(bo[f + 1] - bo[f]), int(ro[f + 1] - ro[f]))
    stats = [w.close() for w in ws]
    assert stats[0]["records"] == n and sum(s["records"] for s in stats[1:]) == n
    for p, body in zip(paths, [c.stream] + c.bucket_body):
        raw = open(p, "rb").read()
        assert raw.endswith(bgzfcases.EOF_BLOCK)
        blocks = bgzfcases.bgzf_blocks(raw)                        # BC field, BSIZE, CRC-32, ISIZE of every block
        assert b"".join(b for b, _ in blocks) == c.header + body, p
    c.free()
    fd.close()


def test_end_to_end_device_full_device_sink(big):
    ref, d, rs = big["ref"], big["d"], big["rs"]
    out = {}
    for records, sink in (("host", "host"), ("device_full", "device")):
        o = os.path.join(d, f"e2e_{records}_{sink}")
        st = e2e.run(ref, [big["files"]], o, pairs_per_batch=1500, bam_threads=2, rec_threads=3, records=records, sink=sink, layout="reference", chunk=fc.CHUNK)
        assert st["pairs"] == rs.n_pairs and st["records"] > 2 * rs.n_pairs and st["batches"] >= 2
        out[records] = (st, {f: rc.inflate(os.path.join(o, f)) for f in st["files"]})
    (sh, fh), (sd, fdev) = out["host"], out["device_full"]
    assert sd["files"] == sh["files"] and sd["records"] == sh["records"]
    for f in sh["files"]:
        assert fdev[f][rc.header_len(fdev[f]):] == fh[f][rc.header_len(fh[f]):], f       # (the header carries the run's time)
    assert len(fh["bc_sorted_bam.bam"]) > 65280


def _tie_cases():
    """every tie of "%.6f": 2 s 10^6 / n an odd integer, n = 128, 256, ... 32768 (a tie needs 128 | n), s <= 4 n"""
    s_all, n_all = [], []
    for n in range(128, 32769, 128):
        s = np.arange(4 * n + 1, dtype=np.int64)
        a = 2000000 * s
        s = s[(a % n == 0) & ((a // n) & 1 == 1)]
        s_all.append(s)
        n_all.append(np.full(len(s), n))
    return np.concatenate(s_all), np.concatenate(n_all)


def test_decimal_text_on_the_device():
    """the device's own %d and %.6f against Python's, on inputs the path does not produce at test size"""
    n = np.repeat(np.arange(1, 513), 4 * np.arange(1, 513) + 1)
    s = np.concatenate([np.arange(4 * k + 1) for k in range(1, 513)])
    ts, tn = _tie_cases()
    assert len(ts) > 100000 and int(((2000000 * ts // tn) % 15625 != 0).sum()) >= 100      # ties whose value is no double
    rng = np.random.default_rng(3)
    rs_, rn = rng.integers(0, 2 ** 31, 100000), rng.integers(1, 60001, 100000)
    s, n = np.concatenate([s, ts, rs_, -rs_[:1000]]), np.concatenate([n, tn, rn, rn[:1000]])
    got = api.selftest_rec_text(s, n)
    want = [b"%.6f" % (int(a) / int(b)) for a, b in zip(s, n)]
    bad = [(int(a), int(b), g, w) for a, b, g, w in zip(s, n, got, want) if g != w]
    assert not bad, bad[:10]
    v = [0, 2 ** 31 - 1, -2 ** 31, -2 ** 31 + 1]
    for k in range(10):
        v += [10 ** k - 1, 10 ** k, 10 ** k + 1, -(10 ** k) + 1, -(10 ** k), -(10 ** k) - 1]
    v = [x for x in v if -2 ** 31 <= x < 2 ** 31] + rng.integers(-2 ** 31, 2 ** 31, 5000).tolist()
    assert api.selftest_rec_text(v) == [b"%d" % x for x in v]

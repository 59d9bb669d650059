"""The records phase on the host test double (arx_batch_records / _fetch / _view, arx_bam_write_encoded; arachne_amd/csrc/dev_records.h,
pipeline_records.h): the BAM-encoded primary records written by the device functors against the EXISTING host path -- arx_recbuf_build ->
arx_bam_write on a host writer, the file inflated block by block -- on a crafted FASTQ workload (tests/reccases.py) read through the feeder.
Everything is byte-exact.  GPU variant: tests/test_device_records_gpu.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from arachne_amd import api, e2e, synth
import reccases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "hostsim", "libarx_hostsim.so")
NOT_UNIQUE = {"AAAT-1"}


@pytest.fixture(scope="module")
def world(built):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    d = tempfile.mkdtemp(prefix="arx_rec_")
    g = synth.make_genome(31, [300000])
    fa = rc.make_index(d, g, SIM)
    pairs = rc.crafted_pairs(g)
    f1, f2 = os.path.join(d, "c1.fq"), os.path.join(d, "c2.fq")
    rc.write_fastq(pairs, f1, f2)
    ref = api.Reference(fa, lib_path=SIM)
    fd = api.Feeder(f1, f2, lib_path=SIM)
    sb, v = fd.next_raw(10 ** 6)
    assert int(v["n_pairs"]) == len(pairs) and int(v["n_sets"]) == 4
    sb, keep = rc.with_unique(sb, v, NOT_UNIQUE)
    case = rc.Case(ref, sb, v, SIM)
    # the reference output, computed once: the host path's file with and without duplicate flags
    host = {}
    for dup in (True, False):
        data = rc.host_file(os.path.join(d, f"host{int(dup)}.bam"), ref, SIM, [case.host_view(dup)])
        host[dup] = (data, rc.header_len(data))
    w = dict(d=d, g=g, pairs=pairs, files=(f1, f2), ref=ref, fd=fd, sb=sb, v=v, keep=keep, case=case, host=host)
    yield w
    case.free()
    fd.close()
    ref.close()


def test_workload_covers_every_record_class(world):
    """on the host path's records: the workload reaches every rule the device code restates"""
    data, h = world["host"][True]
    off, recs = rc.walk(data[h:])
    ap = world["case"].active_pos()
    assert len(recs) == 2 * len(world["pairs"]) == len(ap)
    assert any(r["flag"] & 4 and p == -1 for r, p in zip(recs, ap)), "no placeholder record"
    assert any(r["flag"] & 4 and p != -1 for r, p in zip(recs, ap)), "no record unmapped by the score rule"
    assert any(r["flag"] & 0x10 for r in recs) and any(not r["flag"] & 0x10 for r in recs)
    assert any(r["flag"] & 0x400 for r in recs), "no duplicate"
    ops = set().union(*[r["ops"] for r in recs])
    assert {0, 1, 2, 4} <= ops, ops
    assert {r["l_seq"] & 1 for r in recs} == {0, 1} and any(r["l_seq"] == 0 for r in recs)
    assert {r["l_seq"] for r in recs} >= {18, 255}
    assert any(r["aux"].startswith(b"RGZ") for r in recs) and any(r["aux"].startswith(b"ASi") for r in recs)
    assert any(b"BXZ" in r["aux"] for r in recs) and any(b"BXZ" not in r["aux"] for r in recs)
    assert {r["l_name"] - 1 for r in recs} >= {1, 254} and {(r["l_name"] - 1) % 16 for r in recs} == set(range(16))
    assert set((off[:-1] % 16).tolist()) == set(range(16))
    # the duplicate flags are the only difference between the two reference files
    d0, h0 = world["host"][False]
    assert d0 != data and len(d0) == len(data)


@pytest.mark.parametrize("dup", [True, False])
def test_stream_is_the_host_paths(world, dup):
    data, h = world["host"][dup]
    b = world["case"].batch
    n, nb = b.records(world["sb"], dup=dup)
    assert (n, nb) == (2 * len(world["pairs"]), len(data) - h)
    stream, off = b.records_fetch()
    assert stream.tobytes() == data[h:]
    assert np.array_equal(off, rc.walk(data[h:])[0])
    p = os.path.join(world["d"], f"enc{int(dup)}.bam")
    w = rc.open_writer(p, world["ref"], SIM)
    w.write_encoded(stream, n)
    st = w.close()
    assert st["records"] == n and rc.inflate(p) == data
    # the view: in the test double device memory is host memory
    ptr, vb, vn = b.records_view()
    assert (vb, vn) == (nb, n) and C.string_at(ptr, vb) == data[h:]


def test_one_pair(world):
    ref = world["ref"]
    d = world["d"]
    f1, f2 = os.path.join(d, "o1.fq"), os.path.join(d, "o2.fq")
    rc.write_fastq(world["pairs"][:1], f1, f2)
    fd = api.Feeder(f1, f2, lib_path=SIM)
    sb, v = fd.next_raw(10)
    c = rc.Case(ref, sb, v, SIM)
    data = rc.host_file(os.path.join(d, "o.bam"), ref, SIM, [c.host_view(True)])
    assert c.batch.records(sb) [0] == 2
    assert c.batch.records_fetch()[0].tobytes() == data[rc.header_len(data):]
    c.free()
    fd.close()


def test_two_batches_and_interleaved_writes(world):
    """the same reads as two super-batches into one writer: the carry (the bytes short of a BGZF block) crosses the write_encoded boundary; then a
    host write_view and a write_encoded interleaved on one writer"""
    ref, d = world["ref"], world["d"]
    fd = api.Feeder(*world["files"], lib_path=SIM)
    views, streams, cases = [], [], []
    while True:
        nx = fd.next_raw(30)
        if nx is None:
            break
        sb, v = nx
        sb, keep = rc.with_unique(sb, v, NOT_UNIQUE)
        c = rc.Case(ref, sb, v, SIM)
        n, nb = c.batch.records(sb)
        streams.append((c.batch.records_fetch()[0].copy(), n))
        views.append(c.host_view(True))
        cases.append((c, keep))
    assert len(streams) >= 2
    want = rc.host_file(os.path.join(d, "two_host.bam"), ref, SIM, views)
    assert want == world["host"][True][0]          # whole barcode sets: the batching does not show in the records
    p = os.path.join(d, "two_enc.bam")
    w = rc.open_writer(p, ref, SIM)
    for s, n in streams:
        w.write_encoded(s, n)
    assert w.close()["records"] == 2 * len(world["pairs"])
    assert rc.inflate(p) == want
    p = os.path.join(d, "mixed.bam")
    w = rc.open_writer(p, ref, SIM)
    for k, (s, n) in enumerate(streams):
        if k & 1:
            w.write_view(views[k])
        else:
            w.write_encoded(s, n)
    w.close()
    assert rc.inflate(p) == want
    for c, keep in cases:
        c.free()
    fd.close()


def test_lifetime(world):
    lib = C.CDLL(SIM)
    lib.arx_test_arena_live_bytes.restype = C.c_int64
    lib.arx_test_arena_live_bytes.argtypes = [C.c_void_p]
    ref, sb, v = world["ref"], world["sb"], world["v"]
    b = ref.batch(v["bases"], v["lens"])
    with pytest.raises(api.ArachneError, match="arx_batch_records before arx_batch_rfa"):
        b.records(sb)
    b.run()
    with pytest.raises(api.ArachneError, match="arx_batch_records before arx_batch_rfa"):
        b.records(sb, dup=False)
    b.rfa(v["set_pair_off"], v["do_rfa"], fetch=False)
    with pytest.raises(api.ArachneError, match="before arx_batch_post"):
        b.records(sb, dup=True)
    with pytest.raises(api.ArachneError, match="arx_batch_records_fetch before arx_batch_records"):
        b.records_fetch()
    with pytest.raises(api.ArachneError, match="arx_batch_records_view before arx_batch_records"):
        b.records_view()
    assert b.records(sb, dup=False)[0] == 2 * int(v["n_pairs"])       # without post: the phase in between is empty
    b.post(fetch=False)                                                # ... and post discards the records behind it
    with pytest.raises(api.ArachneError, match="arx_batch_records_fetch before"):
        b.records_fetch()
    b.records(sb)
    live = lib.arx_test_arena_live_bytes(b.h)
    first = b.records_fetch()[0].copy()
    b.records(sb)
    assert lib.arx_test_arena_live_bytes(b.h) == live                  # entering the phase again rewinds its own memory
    assert np.array_equal(b.records_fetch()[0], first)
    b.tags(fetch=False)                                                # a phase in front of it, entered later: the records are gone
    with pytest.raises(api.ArachneError, match="arx_batch_records_view before"):
        b.records_view()
    b.records(sb)
    b.rfa(v["set_pair_off"], v["do_rfa"], fetch=False)
    with pytest.raises(api.ArachneError, match="arx_batch_records_fetch before"):
        b.records_fetch()
    b.post(fetch=False)
    b.records(sb)
    b.reset(v["bases"], v["lens"])
    with pytest.raises(api.ArachneError, match="arx_batch_records_fetch before"):
        b.records_fetch()
    b.free()


def _sb_copy(sb):
    sb2 = api._SuperBatch()
    C.memmove(C.byref(sb2), C.byref(sb), C.sizeof(sb))
    return sb2


def test_argument_errors(world):
    ref, sb, v, d = world["ref"], world["sb"], world["v"], world["d"]
    b = world["case"].batch
    P = int(v["n_pairs"])
    # a 255-byte name: the host sink's text for the same fault (record 2p is the pair's first)
    no = np.frombuffer((C.c_int64 * (P + 1)).from_address(sb.name_off), dtype=np.int64).copy()
    names = C.string_at(sb.names, int(no[-1]))
    p = 3
    grow = 255 - int(no[p + 1] - no[p])
    big = names[:no[p + 1]] + b"x" * grow + names[no[p + 1]:]
    no[p + 1:] += grow
    buf = C.create_string_buffer(big, len(big))
    bad = _sb_copy(sb)
    bad.name_off, bad.names = no.ctypes.data, C.addressof(buf)
    with pytest.raises(api.ArachneError, match="read name of record 6 must be 1..254 bytes") as ei:
        b.records(bad)
    assert "error -2" in str(ei.value)
    view = world["case"].host_view(True)
    w = rc.open_writer(os.path.join(d, "n255.bam"), ref, SIM)
    hv = api._BamBatch()
    C.memmove(C.byref(hv), C.byref(view), C.sizeof(view))
    no2 = np.frombuffer((C.c_int64 * (2 * P + 1)).from_address(view.name_off), dtype=np.int64).copy()
    no2[2 * p + 1:] += 255 - int(no2[2 * p + 1] - no2[2 * p])
    hv.name_off = no2.ctypes.data
    with pytest.raises(api.ArachneError, match="read name of record 6 must be 1..254 bytes"):
        w.write_view(hv)                                              # the host sink says the same (checked before it reads a name)
    w.close()
    # the wrong pair count
    bad = _sb_copy(sb)
    bad.n_pairs = P - 1
    with pytest.raises(api.ArachneError, match="2 \\* n_pairs must equal n_reads") as ei:
        b.records(bad)
    assert "error -2" in str(ei.value)
    # a block_size chain that does not tile: ARX_E_ARG, the file as if the call had not been made
    data, h = world["host"][True]
    n, nb = b.records(sb)
    stream = b.records_fetch()[0].copy()
    path = os.path.join(d, "tile.bam")
    w = rc.open_writer(path, ref, SIM)
    for broken, cnt in ((stream[:-1], n), (stream, n - 1), (np.concatenate([stream, np.zeros(3, np.uint8)]), n)):
        with pytest.raises(api.ArachneError, match="arx_bam_write_encoded: the "):
            w.write_encoded(broken, cnt)
    cut = stream.copy()
    cut[0:4] = np.frombuffer(np.int32(20).tobytes(), dtype=np.uint8)  # shorter than a fixed part
    with pytest.raises(api.ArachneError, match="do not tile"):
        w.write_encoded(cut, n)
    assert w.lib.arx_bam_write_encoded(w.h, stream.ctypes.data, len(stream) - 1, n) == -2
    w.write_encoded(stream, n)
    assert w.close()["records"] == n
    assert rc.inflate(path) == data


def test_e2e_records_device(world):
    """e2e.run(records="device") on the workload of test_e2e.py's host-double case: the BAMs inflate to the bytes of records="host" """
    g = synth.make_genome(15, [400000, 150000])
    rs = synth.make_reads(16, g, 6, 60, invalid_frac=0.25)
    rs.seqs[5] = np.random.default_rng(1).integers(0, 4, size=150)
    d = tempfile.mkdtemp(prefix="arx_rec_e2e_")
    fa = rc.make_index(d, g, SIM)
    po = rs.pair_offsets()
    workers = 2
    cuts = [int(po[len(po) * k // workers]) for k in range(workers)] + [rs.n_pairs]
    files = []
    for k in range(workers):
        f1, f2 = os.path.join(d, f"r1_{k}.fq"), os.path.join(d, f"r2_{k}.fq")
        synth.write_fastq_fast(rs, f1, f2, cuts[k], cuts[k + 1])
        files.append((f1, f2))
    ref = api.Reference(fa, lib_path=SIM)
    try:
        kw = dict(pairs_per_batch=max(50, rs.n_pairs // (3 * workers)), bam_threads=2, rec_threads=3, lib_path=SIM)
        sh = e2e.run(ref, files, os.path.join(d, "host"), **kw)
        sd = e2e.run(ref, files, os.path.join(d, "dev"), records="device", **kw)
        assert sd["pairs"] == sh["pairs"] == rs.n_pairs and sd["records"] == sh["records"] == 2 * rs.n_pairs and sd["batches"] == sh["batches"]
        assert set(sd) == set(sh)
        for k in range(workers):
            assert rc.inflate(os.path.join(d, f"dev.{k}.bam")) == rc.inflate(os.path.join(d, f"host.{k}.bam"))
        # the device feeder's loop (one producer, two workers with a file each; which worker takes which super-batch is free): the same records
        recs = {}
        for records in ("host", "device"):
            st = e2e.run(ref, files[:1], os.path.join(d, "f" + records), records=records, feeder="device", workers=2, **kw)
            assert st["pairs"] == cuts[1] and st["records"] == 2 * cuts[1]
            recs[records] = []
            for f in st["files"]:
                data = rc.inflate(f)
                s = data[rc.header_len(data):]
                off = rc.walk(s)[0]
                recs[records] += [s[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        assert sorted(recs["device"]) == sorted(recs["host"]) and len(recs["host"]) == 2 * cuts[1]
        with pytest.raises(ValueError):
            e2e.run(ref, files, os.path.join(d, "x"), records="device", layout="reference", **kw)
        with pytest.raises(ValueError):
            e2e.run(ref, files, os.path.join(d, "x"), records="gpu", **kw)
    finally:
        ref.close()

"""The full records phase on the host test double (arx_batch_records_full, arx_batch_records_buckets_fetch / _view; arachne_amd/csrc/
dev_records_full.h, pipeline_records.h): the reference's record set and its position buckets written by the device functors against the
EXISTING host path -- arx_recbuf_build_full -> arx_bam_write for the stream, arx_bam_write_select into a writer of its own for every bucket,
the files inflated -- on a crafted FASTQ workload (tests/recfullcases.py) read through the feeder, and e2e.run(layout="reference",
records="device_full") against records="host".  Everything is byte-exact.  GPU variant: tests/test_device_records_full_gpu.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from arachne_amd import api, e2e, synth
import reccases as rc
import recfullcases as fc
import test_bam_reference_layout as trl

HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "hostsim", "libarx_hostsim.so")


@pytest.fixture(scope="module")
def world(built):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    d = tempfile.mkdtemp(prefix="arx_recfull_")
    w = fc.World(SIM, d)
    w.case = fc.FullCase(w.ref, w.sb, w.v, w.table, SIM, d, "host")
    yield w
    w.case.free()
    w.close()


def _aux(a):
    """the aux fields of a record -> dict tag -> value bytes (the text of a Z field, the four bytes of an i field)"""
    out, o = {}, 0
    while o < len(a):
        if a[o + 2:o + 3] == b"i":
            out[a[o:o + 2]] = a[o + 3:o + 7]
            o += 7
        else:
            e = a.index(b"\0", o + 3)
            out[a[o:o + 2]] = a[o + 3:e]
            o = e + 1
    return out


def test_workload_covers_every_record_class(world):
    """on the HOST path's records: the workload reaches what the device code restates"""
    c = world.case
    off, recs = rc.walk(c.stream)
    ax = [_aux(r["aux"]) for r in recs]
    sec = [(r, a) for r, a in zip(recs, ax) if r["flag"] & 0x100]
    assert len(recs) == 2 * len(world.pairs) + len(sec) == len(c.bucket)
    assert any(r["flag"] & 0x10 for r, _ in sec) and any(not r["flag"] & 0x10 for r, _ in sec), "split records on one strand only"
    # HardClip: the split record's own CIGAR starts / ends with H (op 5) and it is shorter than its primary
    cig = {}
    for q, r in enumerate(recs):
        if r["flag"] & 0x100:
            o = int(off[q])
            n_cig = int.from_bytes(c.stream[o + 16:o + 18], "little")
            cig[q] = np.frombuffer(c.stream, dtype="<u4", count=n_cig, offset=o + 36 + r["l_name"]) & 15
    assert any(w[0] == 5 for w in cig.values()) and any(w[-1] == 5 for w in cig.values()), "no leading / trailing hard clip"
    assert all(recs[q]["l_seq"] < recs[q - 1]["l_seq"] for q in cig)
    assert any(a[b"XC"] for a in ax if b"XC" in a), "no second best with mismatches"
    n_ac = {a[b"AC"].count(b";") for a in ax}
    assert {0, 1} <= n_ac and max(n_ac) >= 5, n_ac
    sa = [a[b"SA"].split(b",")[3] for a in ax if b"SA" in a]
    assert any(b"I" in s or b"D" in s for s in sa) and any(b"H" in s for s in sa) and any(b"S" in s for s in sa)
    ap = rc.Case.active_pos(c)
    prim = [r for r in recs if not r["flag"] & 0x100]
    assert any(r["flag"] & 4 and p == -1 for r, p in zip(prim, ap)), "no placeholder record"
    assert any(r["flag"] & 4 and not r["flag"] & 8 and p != -1 for r, p in zip(prim, ap)), "no primary the score rule unmaps while its mate stays mapped"
    assert any(r["l_seq"] == 0 for r in recs)
    assert {r["l_name"] - 1 for r in recs} >= {1, 254} and {(r["l_name"] - 1) % 16 for r in recs} == set(range(16))
    assert any(b"BX" in a for a in ax) and any(b"BX" not in a for a in ax)
    assert any(b"RG" not in a for a in ax)
    assert len({a[b"DM"] for a in ax if b"DM" in a}) >= 2, "no DM tag"
    per = np.bincount(c.bucket, minlength=len(world.table.files))
    assert (per > 0).sum() >= 3 and per[-1] > 0 and (per == 0).any(), per
    assert set((off[:-1] % 16).tolist()) == set(range(16))


def test_streams_are_the_host_paths(world):
    c = world.case
    n, nb = fc.check_identity(c)
    # the views: in the test double device memory is host memory
    ptr, vb, vn = c.batch.records_view()
    assert (vb, vn) == (nb, n) and C.string_at(ptr, vb) == c.stream
    gptr, bo, ro = c.batch.records_buckets_view()
    g = c.batch.records_buckets_fetch()
    assert np.array_equal(bo, g["byte_off"]) and np.array_equal(ro, g["rec_off"]) and C.string_at(gptr, nb) == g["grouped"].tobytes()
    # any argument of the fetch may be NULL
    lib = world.ref.lib
    assert lib.arx_batch_records_buckets_fetch(world.ref.h, c.batch.h, None, None, None, None) == 0
    # through a writer: the stream file and every bucket file as the host path writes them
    p = os.path.join(world.d, "enc.bam")
    w = rc.open_writer(p, world.ref, SIM)
    w.write_encoded(c.batch.records_fetch()[0], n)
    assert w.close()["records"] == n and rc.inflate(p) == c.header + c.stream


def test_small_batches(world):
    """the same reads as super-batches of about 20 pairs, and a single pair: every one through the identity check"""
    fd = api.Feeder(*world.files, lib_path=SIM)
    k = 0
    while True:
        nx = fd.next_raw(20 if k else 1)
        if nx is None:
            break
        sb, v = nx
        sb, keep = rc.with_unique(sb, v, fc.NOT_UNIQUE)
        c = fc.FullCase(world.ref, sb, v, world.table, SIM, world.d, "small%d" % k)
        fc.check_identity(c)
        c.free()
        k += 1
    assert k >= 4
    fd.close()


def test_many_blocks_of_the_grouping():
    """4000 pairs (test_bam_reference_layout's reads, chimeras among them) as one super-batch: more than 30 blocks of the grouping, bucket slices
    longer and shorter than a BGZF block"""
    g, rs = trl._reads(20, 200)
    d = tempfile.mkdtemp(prefix="arx_recfull_big_")
    fa = rc.make_index(d, g, SIM)
    f1, f2 = os.path.join(d, "b1.fq"), os.path.join(d, "b2.fq")
    synth.write_fastq_fast(rs, f1, f2)
    ref = api.Reference(fa, lib_path=SIM)
    try:
        names, _, clens, _, _ = ref.contigs()
        table = api.bucket_table(names, clens, fc.CHUNK, lib_path=SIM)
        fd = api.Feeder(f1, f2, lib_path=SIM)
        sb, v = fd.next_raw(10 ** 7)
        c = fc.FullCase(ref, sb, v, table, SIM, d, "host")
        sizes = [len(b) for b in c.bucket_body]
        assert max(sizes) > 65280 and 0 < min(s for s in sizes if s) < 65280, sizes
        n, nb = fc.check_identity(c)
        assert n > 2 * rs.n_pairs and n > 30 * 256
        c.free()
        fd.close()
    finally:
        ref.close()


def test_lifetime(world):
    lib = C.CDLL(SIM)
    lib.arx_test_arena_live_bytes.restype = C.c_int64
    lib.arx_test_arena_live_bytes.argtypes = [C.c_void_p]
    ref, sb, v, table, c = world.ref, world.sb, world.v, world.table, world.case
    b = ref.batch(v["bases"], v["lens"]).run()
    with pytest.raises(api.ArachneError, match="arx_batch_records_full before arx_batch_rfa") as ei:
        b.records_full(sb, table)
    assert "error -2" in str(ei.value)
    b.rfa(v["set_pair_off"], v["do_rfa"], fetch=False)
    with pytest.raises(api.ArachneError, match="arx_batch_records_full before arx_batch_post"):
        b.records_full(sb, table)
    b.tags(fetch=False)
    with pytest.raises(api.ArachneError, match="arx_batch_records_full before arx_batch_post"):
        b.records_full(sb, table)
    b.post(fetch=False)                                                # (discards the tags behind it)
    with pytest.raises(api.ArachneError, match="arx_batch_records_full before arx_batch_tags"):
        b.records_full(sb, table)
    b.tags(fetch=False)
    # the buckets entries need the full call as the last records call
    b.records(sb)
    plain = b.records_fetch()[0].copy()
    b._n_files = len(table.files)
    for call in (b.records_buckets_fetch, b.records_buckets_view):
        with pytest.raises(api.ArachneError, match="needs arx_batch_records_full as the last records call") as ei:
            call()
        assert "error -2" in str(ei.value)
    # records -> records_full -> records on one handle: each gives its own stream, in the same memory
    n, nb = b.records_full(sb, table)
    live = lib.arx_test_arena_live_bytes(b.h)
    assert b.records_fetch()[0].tobytes() == c.stream and np.array_equal(b.records_buckets_fetch()["bucket"], c.bucket)
    b.records_full(sb, table)
    assert lib.arx_test_arena_live_bytes(b.h) == live                  # entering the phase again rewinds its own memory
    assert b.records_fetch()[0].tobytes() == c.stream
    assert b.records(sb)[0] == 2 * int(v["n_pairs"])
    assert np.array_equal(b.records_fetch()[0], plain) and plain.tobytes() != c.stream
    with pytest.raises(api.ArachneError, match="needs arx_batch_records_full as the last records call"):
        b.records_buckets_fetch()
    # a later tags / post / rfa / reset discards the phase
    for later in (lambda: b.tags(fetch=False), lambda: (b.post(fetch=False), b.tags(fetch=False)),
                  lambda: (b.rfa(v["set_pair_off"], v["do_rfa"], fetch=False), b.post(fetch=False), b.tags(fetch=False))):
        b.records_full(sb, table)
        later()
        with pytest.raises(api.ArachneError, match="arx_batch_records_fetch before"):
            b.records_fetch()
        with pytest.raises(api.ArachneError, match="needs arx_batch_records_full"):
            b.records_buckets_view()
    b.records_full(sb, table)
    assert b.records_fetch()[0].tobytes() == c.stream                  # (and after all that the poisoned arena still gives the same bytes)
    b.reset(v["bases"], v["lens"])
    with pytest.raises(api.ArachneError, match="needs arx_batch_records_full"):
        b.records_buckets_fetch()
    b.free()


def test_argument_errors(world):
    ref, sb, v, c = world.ref, world.sb, world.v, world.case
    b = c.batch
    names, _, clens, _, _ = ref.contigs()
    # a table of another index: one contig fewer
    short = api.bucket_table(names[:1], clens[:1], fc.CHUNK, lib_path=SIM)
    with pytest.raises(api.ArachneError, match="the layout has 1 contigs, the index 2") as ei:
        b.records_full(sb, short)
    assert "error -2" in str(ei.value)
    # a chunk smaller than the table was made for: a bucket outside the table
    bad = api.bucket_table(names, clens, fc.CHUNK, lib_path=SIM)
    bad.chunk = 1000
    with pytest.raises(api.ArachneError, match="bucket lies outside the table") as ei:
        b.records_full(sb, bad)
    assert "error -2" in str(ei.value)
    bad = api.bucket_table(names, clens, fc.CHUNK, lib_path=SIM)
    bad.contig_file[1] = len(bad.files) - 1
    with pytest.raises(api.ArachneError, match="contig_file is not arx_bucket_table's"):
        b.records_full(sb, bad)
    # more files than the grouping's table holds
    many = api.bucket_table(names, clens, 64, lib_path=SIM)
    assert len(many.files) > 4096
    with pytest.raises(api.ArachneError, match="the grouping holds at most 4096") as ei:
        b.records_full(sb, many)
    assert "error -2" in str(ei.value)
    # the super-batch checks of arx_batch_records
    wrong = api._SuperBatch()
    C.memmove(C.byref(wrong), C.byref(sb), C.sizeof(sb))
    wrong.n_pairs = int(v["n_pairs"]) - 1
    with pytest.raises(api.ArachneError, match="2 \\* n_pairs must equal n_reads"):
        b.records_full(wrong, world.table)
    # none of the refusals left anything behind: the batch still gives the host path's streams
    fc.check_identity(c)


def test_split_of_another_read_is_refused(world):
    """arx_recbuf_build_full refuses such a batch with a text; the device raises an error bit that becomes the same ARX_E_ARG"""
    c = world.case
    split = c.post["split"].copy()
    r = int(np.flatnonzero(split["split"] >= 0)[0])
    other = r + 2 if r + 2 < len(split) else r - 2
    split["split"][r] = c.buf["cand_off"][other]
    b = c.buf
    with pytest.raises(api.ArachneError, match="arx_split names a candidate of another read"):
        c.rb.build_full(c.sb, b["cand_off"], b["cands"], b["alns"], b["cigars"], c.post["post"], split, c.post["mm_ref"], c.post["mm_read"], c.tags, c.table, threads=2)
    c.rb.build_full(c.sb, b["cand_off"], b["cands"], b["alns"], b["cigars"], c.post["post"], c.post["split"], c.post["mm_ref"], c.post["mm_read"], c.tags, c.table, threads=2)


def _e2e_world(workers):
    g, rs = trl._reads(5, 60)
    d = tempfile.mkdtemp(prefix="arx_recfull_e2e_")
    fa = rc.make_index(d, g, SIM)
    po = rs.pair_offsets()
    cuts = [int(po[len(po) * k // workers]) for k in range(workers)] + [rs.n_pairs]
    files = []
    for k in range(workers):
        f1, f2 = os.path.join(d, f"r1_{k}.fq"), os.path.join(d, f"r2_{k}.fq")
        synth.write_fastq_fast(rs, f1, f2, cuts[k], cuts[k + 1])
        files.append((f1, f2))
    return g, rs, d, fa, files


def test_e2e_one_worker_is_identical_and_holds_against_the_restatement():
    g, rs, d, fa, files = _e2e_world(1)
    ref = api.Reference(fa, lib_path=SIM)
    try:
        kw = dict(pairs_per_batch=max(50, rs.n_pairs // 3), bam_threads=2, rec_threads=3, lib_path=SIM, layout="reference", chunk=fc.CHUNK, read_groups="S1:L1:1:FC:1")
        sh = e2e.run(ref, files, os.path.join(d, "host"), **kw)
        sd = e2e.run(ref, files, os.path.join(d, "dev"), records="device_full", **kw)
        assert sd["files"] == sh["files"] and len(sh["files"]) >= 4
        assert (sd["pairs"], sd["records"], sd["batches"]) == (sh["pairs"], sh["records"], sh["batches"]) and sd["records"] > 2 * rs.n_pairs and set(sd) == set(sh)
        n_nonempty = 0
        for f in sh["files"]:
            a, b = rc.inflate(os.path.join(d, "host", f)), rc.inflate(os.path.join(d, "dev", f))
            # the header carries the run's time (DT:): the records behind it are what must be identical
            assert a[rc.header_len(a):] == b[rc.header_len(b):], f
            n_nonempty += len(a) > rc.header_len(a)
        assert n_nonempty >= 4
        # bc_sorted_bam.bam against the Python restatement of DoDumpToBam
        names, offs, clens, alt, l_pac = ref.contigs()
        table = api.bucket_table(names, clens, fc.CHUNK, lib_path=SIM)
        po = rs.pair_offsets()
        flags = [api.worth_running_rfa(rs.barcodes[b], int(po[b + 1] - po[b])) for b in range(len(po) - 1)]
        b = ref.batch(rs.seqs, rs.lens).run()
        fo = b.fetch()
        c = b.rfa(po, flags)
        pp = b.post()
        tags = b.tags()
        b.free()
        exp = trl._expected(rs, names, table, c["cands"], c["cand_off"], fo["alns"], fo["cigars"], pp["post"], pp["split"], pp["mm_ref"], pp["mm_read"], tags)
        text, got = trl._read_bam(os.path.join(d, "dev", "bc_sorted_bam.bam"))
        assert len(got) == len(exp) == sd["records"]
        for rec, (bk, e) in zip(got, exp):
            for key in e:
                assert rec[key] == e[key], (e["name"], key, rec[key], e[key])
        with pytest.raises(ValueError, match="layout='reference' needs records='host'"):
            e2e.run(ref, files, os.path.join(d, "x"), records="device", **kw)
        kw["layout"] = "workers"
        with pytest.raises(ValueError, match="records='device_full'"):
            e2e.run(ref, files, os.path.join(d, "x"), records="device_full", **kw)
    finally:
        ref.close()


def test_e2e_several_workers_write_the_same_records():
    """three workers, and the device feeder with two: per file the same multiset of records as records="host" """
    g, rs, d, fa, files = _e2e_world(3)
    ref = api.Reference(fa, lib_path=SIM)
    try:
        kw = dict(pairs_per_batch=max(50, rs.n_pairs // 9), bam_threads=2, rec_threads=3, lib_path=SIM, layout="reference", chunk=fc.CHUNK)
        for tag, extra, fl in (("w3", dict(), files), ("df", dict(feeder="device", workers=2), files[:1])):
            sh = e2e.run(ref, fl, os.path.join(d, tag + "_host"), **kw, **extra)
            sd = e2e.run(ref, fl, os.path.join(d, tag + "_dev"), records="device_full", **kw, **extra)
            assert sd["files"] == sh["files"] and (sd["pairs"], sd["records"]) == (sh["pairs"], sh["records"]) and sd["records"] > 2 * sd["pairs"]
            total = 0
            for f in sh["files"]:
                a, b = fc.records_of(os.path.join(d, tag + "_host", f)), fc.records_of(os.path.join(d, tag + "_dev", f))
                assert sorted(a) == sorted(b), f
                total += len(a)
            assert total == 2 * sh["records"]
    finally:
        ref.close()

"""The index a writer builds of what it is handed, on the GPU (arx_selftest_bam_index_feeds, arx_bam_open_indexed, arx_bam_close_indexed;
arachne_amd/csrc/dev_bamindex.h: BiPush, hip_bamindex.h: BiWriterTap).  1. the cases tests/test_bam_index_feeds_sim.py runs through the host
program -- baicases', csicases' and the block-edge cases of bixcases.py, in a writer's layout under irregular file offsets -- through the
kernels, fed as one feed, per record and in feeds of 61 bytes: held byte for byte to the serial restatement and to what
arx_selftest_bam_index(_csi) gives on the same table; 2. what is refused; 3. files: e2e.finalize(index_pass="writer") against the plain
finalize and arx_bam_index / arx_bam_index_csi of the finished file, writers fed from the host, an empty writer, a refused append, and the
contig above 2^29."""
import os

import numpy as np
import pytest

import baicases as bc
import bgzfio
import bixcases as bx
import csicases as cc
import recfullcases as fc
from arachne_amd import api, e2e
from test_bam_index_gpu import LENS, NAMES, REGIONS, _query_check, _record_set, layout  # noqa: F401  (layout: the fixture)

pytestmark = pytest.mark.gpu
CUTS = ("one", "record", "by61")
# the cases that also run in pieces of 128 bytes (every case does in the host program): long streams, long records, cut fields, borders, a refusal
PIECED = ("records_257", "runs_257", "longer_than_a_slab", "block_size_cut", "slab_cuts_cigar", "level_borders", "every_op", "placed_unmapped", "refuse_order_at_slab_border",
          "bai_records_257", "bai_runs_257", "bai_longer_than_a_slab", "level_borders_depth6", "loffset_backfilled", "bins_65536_apart_two_contigs", "shift_10")


def _feeds(k, ends, **kw):
    return api.selftest_bam_index_feeds(k.stream, k.hdr, k.ref_len, k.at, ends, min_shift=-1 if k.min_shift is None else k.min_shift, **kw)


def _file_pass(k):
    """what the pass over the finished file gives on the same table"""
    if k.min_shift is None:
        return api.selftest_bam_index(k.stream, k.hdr, k.ref_len, k.at, k.isize, 256)
    return api.selftest_bam_index_csi(k.stream, k.hdr, k.ref_len, k.at, k.isize, 256, min_shift=k.min_shift)


def _held(name, k, cuts, segs, pieces):
    for cut in cuts:
        for seg in segs:
            for piece in pieces:
                code, out, st = _feeds(k, cuts[cut], seg_bytes=seg, piece_bytes=piece)
                if k.refused is None:
                    assert code == 0 and out == k.want, (name, cut, seg, piece)
                    assert st["records"] == len(k.recs), (name, cut, seg, piece)
                else:
                    assert code == k.refused.code and out == b"", (name, cut, seg, piece)
                    if k.refused.record is not None:
                        assert (st["refused"] >> 8, st["refused"] & 0xff) == (k.refused.record, k.refused.rule), (name, cut, seg, piece)
    if k.refused is None:
        assert _file_pass(k)[:2] == (0, k.want), name


# ---- 1. the kernels
@pytest.mark.parametrize("seg", bc.SEGS)
def test_bai_cases_through_the_kernels(seg):
    for name, case in bc.cases().items():
        k = bx.relaid(case)
        cuts = bx.cuttings(k)
        _held(name, k, {c: cuts[c] for c in CUTS}, (seg,), (128, 0) if seg == 256 and name in PIECED else (0,))


def test_csi_cases_through_the_kernels():
    for name, case in cc.cases().items():
        if case.min_shift < 0:
            continue                                             # (-1 asks this entry for the .bai)
        k = bx.relaid(case, case.min_shift, seed=7)
        cuts = bx.cuttings(k)
        _held(name, k, {c: cuts[c] for c in CUTS}, (256,), (128, 0) if name in PIECED else (0,))


@pytest.mark.parametrize("name", list(bx.edges()))
def test_block_edges(name):
    k = bx.edges()[name]
    cuts = bx.edge_cuttings(name, k)
    _held(name, k, cuts, (4096,), (128, 0) if name == "run_across_pieces" else (1000, 0))
    k2 = bx.Laid(k.recs, k.ref_len, k.hdr, 14, seed=3)
    _held(name, k2, {"record": cuts["record"]}, (4096,), (0,))


# ---- 2. what is refused
def test_an_order_offence_across_a_feed_border_names_the_record():
    k = bx.relaid(bc.cases()["refuse_order_at_slab_border"])
    assert (k.refused.record, k.refused.rule) == (4, bc.R_ORDER)
    for ends in ([k.off[4], len(k.stream)], [k.off[4] + 9, len(k.stream)], bx.cuttings(k)["record"]):     # the offender: a feed's first record, cut by one, alone in one
        code, out, st = _feeds(k, ends, seg_bytes=64)
        assert code == api.ARX_E_ARG and out == b"" and (st["refused"] >> 8, st["refused"] & 0xff) == (4, bc.R_ORDER)


def test_the_other_record_rules_and_broken_chains():
    for name, rule in (("refuse_refid_n_ref", bc.R_REFID), ("refuse_refid_minus_2", bc.R_REFID), ("refuse_negative_pos", bc.R_POS), ("refuse_end_beyond_contig", bc.R_END)):
        k = bx.relaid(bc.cases()[name])
        for ends in bx.cuttings(k).values():
            code, out, st = _feeds(k, ends, seg_bytes=64)
            assert code == api.ARX_E_ARG and st["refused"] & 0xff == rule and st["refused"] >> 8 == k.refused.record, name
    for name, case in bc.broken().items():
        k = bx.relaid(case)
        for ends in bx.cuttings(k).values():
            assert _feeds(k, ends, seg_bytes=64)[:2] == (api.ARX_E_IO, b""), name                           # last_record_past_the_end: the stream ends inside a record


def test_bad_arguments_and_a_small_buffer():
    k = bx.relaid(bc.cases()["one_record"])
    n = len(k.stream)
    assert _feeds(k, [n], seg_bytes=96)[0] == api.ARX_E_ARG                                               # no power of two
    assert _feeds(k, [n - 1], seg_bytes=64)[0] == api.ARX_E_ARG                                           # the last feed does not end the stream
    assert _feeds(k, [20, 10, n], seg_bytes=64)[0] == api.ARX_E_ARG                                       # not ascending
    assert _feeds(k, [], seg_bytes=64)[0] == api.ARX_E_ARG
    assert _feeds(k, [n], seg_bytes=64, piece_bytes=-1)[0] == api.ARX_E_ARG
    assert api.selftest_bam_index_feeds(k.stream, k.hdr, k.ref_len, k.at + [k.at[-1] + 30], [n], 64)[0] == api.ARX_E_ARG          # one block more than the layout has
    assert api.selftest_bam_index_feeds(k.stream, k.hdr, k.ref_len, k.at[:1] + k.at[:-1], [n], 64)[0] == api.ARX_E_ARG           # offsets that do not ascend
    assert api.selftest_bam_index_feeds(k.stream, k.hdr, k.ref_len, [a + (1 << 48) for a in k.at], [n], 64)[0] == api.ARX_E_ARG
    assert api.selftest_bam_index_feeds(k.stream, k.hdr, k.ref_len, k.at, [n], 64, min_shift=9)[0] == api.ARX_E_ARG
    assert api.selftest_bam_index_feeds(k.stream, k.hdr, [(1 << 29) + 1], k.at, [n], 64)[0] == api.ARX_E_ARG                      # the .bai of a long contig
    code, out, _ = _feeds(k, [n], seg_bytes=64, out_cap=len(k.want) - 1)
    assert code == api.ARX_E_TOO_LARGE and out == b""
    assert _feeds(k, [n], seg_bytes=64, out_cap=len(k.want))[1] == k.want


# ---- 3. files
def _index_of(path, fmt):
    """(what the writer wrote, what the pass over the finished file writes), the .csi's inflated"""
    own = open(path + "." + fmt, "rb").read()
    again = path + ".again." + fmt
    (api.bam_index_csi if fmt == "csi" else api.bam_index)(path, again)
    both = own, open(again, "rb").read()
    return tuple(bgzfio.inflate(x) for x in both) if fmt == "csi" else both


def test_finalize_with_the_index_in_the_writer(layout):
    ref, d, out = layout
    names, offs, clens, alt, l_pac = ref.contigs()
    for sink in ("host", "device"):
        plain_path = os.path.join(d, "w_plain_%s.bam" % sink)
        plain = e2e.finalize(ref, out, plain_path, sink=sink, chunk=fc.CHUNK, bam_threads=2)
        want_raw = open(plain_path, "rb").read()
        for fmt in ("bai", "csi"):
            p = os.path.join(d, "w_%s_%s.bam" % (sink, fmt))
            fin = e2e.finalize(ref, out, p, sink=sink, chunk=fc.CHUNK, bam_threads=2, index=fmt, index_pass="writer")
            assert sorted(fin) == sorted(list(plain) + ["index", "index_seconds", "index_format"]) and fin["index_format"] == fmt
            assert fin["records"] == plain["records"] == fin["index"]["records"] > 0 and fin["index"]["read_us"] == fin["index"]["inflate_us"] == 0
            assert open(p, "rb").read() == want_raw, (sink, fmt)                                          # byte for byte the file without an index
            own, again = _index_of(p, fmt)
            assert own == again, (sink, fmt)
            assert not os.path.exists(p + "." + fmt + ".tmp")
            if fmt == "bai":
                recs = fc.records_of(p)
                regions = [q for i, l in enumerate(clens) for q in ((i, 0, l), (i, l // 2, l // 2 + 1), (i, l - 1, l), (i, max(0, min(l, 16384) - 1), min(l, 16385)))]
                _query_check(own, want_raw, recs, clens, regions)


def _plain_and_indexed(ref, d, tag, feed, device, fmt="bai", **kw):
    """the same appends into a writer without and with the index -> (path of the indexed file, its close's answer)"""
    paths = [os.path.join(d, "%s_%s_%d.bam" % (tag, x, device)) for x in ("plain", "indexed")]
    w = api.BamWriter(paths[0], NAMES, LENS, extra_header="@PG\tID:t\n", threads=2, level=1, device=ref if device else None, coordinate=True)
    feed(w)
    w.close()
    w = api.BamWriter(paths[1], NAMES, LENS, extra_header="@PG\tID:t\n", threads=2, level=1, device=ref if device else None, index=fmt, index_device=ref, **kw)
    feed(w)
    st = w.close()
    assert open(paths[0], "rb").read() == open(paths[1], "rb").read()
    return paths[1], st


def test_writers_fed_from_the_host(layout):
    ref, d, _ = layout
    recs = _record_set()

    def encoded(w):
        for a in range(0, len(recs), 900):
            w.write_encoded(b"".join(recs[a:a + 900]), len(recs[a:a + 900]))

    def batches(w):                                              # arx_bam_write: the sink encodes; every record an unplaced one with a name of its own
        for a in range(0, 300, 70):
            n = min(70, 300 - a)
            w.write([b"r%d" % (a + j) for j in range(n)], np.full(n, 4), np.full(n, -1), np.full(n, -1), np.zeros(n), np.full(n, -1), np.full(n, -1), np.zeros(n),
                    [np.zeros(0, np.uint32)] * n, [b"ACGT" * (1 + (a + j) % 200) for j in range(n)], [b"I" * (4 * (1 + (a + j) % 200)) for j in range(n)], [b""] * n)

    for device in (False, True):
        for fmt in ("bai", "csi"):
            p, st = _plain_and_indexed(ref, d, "enc_" + fmt, encoded, device, fmt)
            own, again = _index_of(p, fmt)
            assert own == again and st["index"]["records"] == len(recs) and st["index"]["n_no_coor"] == 77 and st["index_format"] == fmt
            if fmt == "bai":
                raw = open(p, "rb").read()
                bai, hits = _query_check(own, raw, recs, LENS, REGIONS)
                assert hits > len(recs) and st["index"]["blocks"] == len(bgzfio.split(raw)) - 1 > 8       # (the EOF block is not counted)
        p, st = _plain_and_indexed(ref, d, "bat", batches, device)
        own, again = _index_of(p, "bai")
        assert own == again and st["index"]["records"] == st["index"]["n_no_coor"] == 300
        p, st = _plain_and_indexed(ref, d, "none", lambda w: None, device)                                # closed with nothing appended
        own, again = _index_of(p, "bai")
        assert own == again and st["index"]["records"] == 0 and bc.read_bai(own)["refs"] == [dict(bins={}, pseudo=None, lin=[])] * 4


def test_a_refused_append_leaves_a_complete_bam_and_no_index(layout):
    ref, d, _ = layout
    recs = _record_set()
    for device in (False, True):
        p = os.path.join(d, "refused_%d.bam" % device)
        w = api.BamWriter(p, NAMES, LENS, threads=2, level=1, device=ref if device else None, index="bai", index_device=ref)
        w.write_encoded(b"".join(recs[:2000]), 2000)
        with pytest.raises(api.ArachneError) as e:
            w.write_encoded(b"".join(recs[100:200]), 100)                                                 # record 2000 is smaller than its predecessor
        assert e.value.code == api.ARX_E_ARG and "record 2000" in str(e.value) and "sorted" in str(e.value)
        w.write_encoded(b"".join(recs[2000:]), len(recs) - 2000)                                          # the writer goes on as a plain one
        with pytest.raises(api.ArachneError) as e:
            w.close()
        assert e.value.code == api.ARX_E_ARG and "the BAM is complete" in str(e.value) and "index was not written" in str(e.value)
        assert not os.path.exists(p + ".bai") and not os.path.exists(p + ".bai.tmp")
        assert fc.records_of(p) == recs                                                                   # nothing of the refused append is in the file
        for bad, rule in ((bc.m(4, 5, b"r"), "refID"), (bc.m(0, -1, b"n"), "pos < 0"), (bc.m(3, 2995, b"e", "6M"), "beyond")):
            q = os.path.join(d, "rule_%d.bam" % device)
            w = api.BamWriter(q, NAMES, LENS, threads=1, level=1, device=ref if device else None, index="auto", index_device=ref)
            with pytest.raises(api.ArachneError) as e:
                w.write_encoded(bad, 1)
            assert e.value.code == api.ARX_E_ARG and "record 0" in str(e.value) and rule in str(e.value)
            with pytest.raises(api.ArachneError):
                w.close()
            assert fc.records_of(q) == [] and not os.path.exists(q + ".bai")


def test_a_contig_above_2_29(layout):
    ref, d, _ = layout
    p = os.path.join(d, "long_contig.bam")
    with pytest.raises(api.ArachneError) as e:
        api.BamWriter(p, ["big"], [(1 << 29) + 1], threads=1, index="bai", index_device=ref)
    assert e.value.code == api.ARX_E_ARG and "CSI" in str(e.value) and not os.path.exists(p)              # refused at open: nothing is created
    w = api.BamWriter(p, ["big"], [(1 << 29) + 1], threads=1, level=1, index="auto", index_device=ref)
    recs = [bc.m(0, 5, b"a"), bc.m(0, (1 << 29) - 9, b"b")]                                               # the second ends at the contig's last base
    w.write_encoded(b"".join(recs), 2)
    st = w.close()
    assert st["index_format"] == "csi" and st["index"]["depth"] == 6 and os.path.exists(p + ".csi") and not os.path.exists(p + ".bai")
    own, again = _index_of(p, "csi")
    assert own == again and cc.read_csi(own)["depth"] == 6
    with pytest.raises(api.ArachneError) as e:
        api.BamWriter(p + ".x", ["c"], [1000], threads=1, index="csi", min_shift=9, index_device=ref)
    assert e.value.code == api.ARX_E_ARG
    with pytest.raises(ValueError):
        api.BamWriter(p + ".x", ["c"], [1000], threads=1, index="bai")                                   # no GPU named

"""The .csi of a coordinate-sorted BAM file on the GPU (arx_bam_index_csi, arx_selftest_bam_index_csi; arachne_amd/csrc/dev_bamindex.h under a
CSI scheme, hip_bamindex.h).  1. the cases of csicases.py -- the ones tests/test_bam_index_csi_sim.py runs through the host program -- through
the kernels, at every segment and slab size, held byte for byte to csicases.csi_of (and, where a .bai exists, to baicases.bai_of's bins, chunks
and linear index); 2. real files with a contig of 2^31 - 1 bases from both sinks, indexed as one slab and a block per slab, the file held to
BGZF's form, its inflated bytes to csi_of over the file's own block table, and the index queried by the independent reader on both sides of 2^29
and 2^30; 3. e2e.finalize(index="csi" / "auto"); 4. the .bai's refusal of the long contig, which names the call that is not refused."""
import os

import numpy as np
import pytest

import baicases as bc
import bgzfio
import csicases as cc
import reccases as rc
import recfullcases as fc
from test_bam_index_gpu import _table, layout  # noqa: F401 -- the reference-layout directory of the .bai's test
from arachne_amd import api, e2e

pytestmark = pytest.mark.gpu


def _index(case, seg, slab, min_shift=None, **kw):
    return api.selftest_bam_index_csi(case.stream, case.hdr, case.ref_len, case.at, case.isize, seg, slab, case.min_shift if min_shift is None else min_shift, **kw)


# ---- 1. the kernels on streams with a block table
@pytest.mark.parametrize("seg", cc.SEGS)
def test_cases_through_the_kernels(seg):
    for name, case in cc.cases().items():
        for slab in case.slabs:
            code, csi, st = _index(case, seg, slab)
            if case.refused is None:
                assert code == 0 and csi == case.want, (name, slab)
                assert (st["min_shift"], st["depth"]) == cc.scheme(case.min_shift, case.ref_len), (name, slab)
                assert st["records"] == len(case.recs) and st["n_no_coor"] == cc.read_csi(csi)["n_no_coor"], (name, slab)
            else:
                assert code == case.refused.code and csi == b"", (name, slab)
                if case.refused.record is not None:
                    assert (st["refused"] >> 8, st["refused"] & 0xff) == (case.refused.record, case.refused.rule), (name, slab)
        if case.refused is None and case.min_shift == 14 and max(case.ref_len, default=0) <= cc.BAI_MAX:
            cc.same_as_bai(_index(case, seg, 0)[1], case.bai)                        # expected values that csi_of had no part in
        if name.startswith("slab_cuts") or name in ("longer_than_a_slab", "block_size_cut"):
            assert _index(case, seg, case.slabs[0])[2]["slabs"] >= 2


@pytest.mark.parametrize("seg", cc.SEGS)
def test_broken_chains_are_refused(seg):
    for name, case in bc.broken().items():
        for slab in case.slabs:
            code, csi, st = _index(case, seg, slab, 14)
            assert code == api.ARX_E_IO and csi == b"", (name, slab)


def test_bad_arguments_and_a_small_buffer():
    case = cc.cases()["depth6_at_2_31_minus_1"]
    for min_shift in (9, 25, -1):
        assert _index(case, 64, 0, min_shift)[0] == api.ARX_E_ARG
    assert _index(case, 96, 0)[0] == api.ARX_E_ARG                                                                       # no power of two
    code, csi, st = _index(case, 64, 0, out_cap=len(case.want) - 1)
    assert code == api.ARX_E_TOO_LARGE and csi == b""
    assert _index(case, 64, 0, out_cap=len(case.want))[1] == case.want
    assert _index(case, 64, 0, 0)[1] == case.want                                                                        # 0 means 14


# ---- 2. files
NAMES, LENS = ["big", "small"], [cc.TOP, 70000]
P29, P30 = 1 << 29, 1 << 30


def _record_set():
    """about 2,000 sorted records, half of them above 2^29, some spliced across 2^29 and 2^30; read lengths mixed so that blocks end inside records"""
    rng = np.random.default_rng(23)
    where = np.concatenate([rng.integers(0, 3000000, 500), rng.integers(P29 - 200000, P29 - 300, 350), rng.integers(P29, P29 + 400000, 350), rng.integers(P30 - 300000, P30 - 300, 250),
                            rng.integers(P30, P30 + 300000, 250), rng.integers(cc.TOP - 200000, cc.TOP - 700, 200)])
    recs = []
    for k, pos in enumerate(sorted(int(x) for x in where)):
        l = int(rng.integers(30, 260))
        if k % 97 == 5 and P29 - 200000 <= pos < P29:
            recs.append(bc.m(0, pos, b"n29_%d" % k, "%dM%dN%dM" % (10, 300000 + 11 * k, l - 10), l_seq=l))                 # across 2^29
        elif k % 89 == 7 and P30 - 300000 <= pos < P30:
            recs.append(bc.m(0, pos, b"n30_%d" % k, "%dM%dN%dM" % (10, 400000 + 13 * k, l - 10), l_seq=l))                 # across 2^30
        elif k % 9 == 0:
            recs.append(bc.rec(0, pos, b"u%d" % k, l_seq=l, flag=4 | 1))                                                  # placed with its mate
        elif k % 9 == 1:
            recs.append(bc.m(0, pos, b"d%d" % k, "%dS%dM%dD%dM" % (5, l - 25, 3 + k % 300, 20), l_seq=l))
        else:
            recs.append(bc.m(0, pos, b"m%d" % k, "%dM" % l, l_seq=l))
    recs += [bc.m(1, int(p), b"s%d" % k, "40M", l_seq=40) for k, p in enumerate(sorted(rng.integers(0, 69000, 100)))]
    recs += [bc.rec(-1, -1, b"x%d" % k, l_seq=int(rng.integers(20, 200)), flag=4) for k in range(41)]
    keys = [(bc.fields(r)[1] & 0xFFFFFFFF, bc.fields(r)[2]) for r in recs]
    assert keys == sorted(keys) and all(bc.interval(r)[1] <= LENS[bc.fields(r)[1]] for r in recs[:-41])
    assert sum(1 for r in recs if bc.fields(r)[1] == 0 and bc.fields(r)[2] >= P29) >= 950
    assert sum(1 for r in recs if bc.interval(r)[0] < P29 < bc.interval(r)[1]) >= 2 and sum(1 for r in recs if bc.interval(r)[0] < P30 < bc.interval(r)[1]) >= 2
    return recs


REGIONS = [(0, 0, cc.TOP), (0, 0, 1), (0, 16383, 16385), (0, 1000000, 2000000), (0, 2999000, 3000400), (0, P29 - 1, P29), (0, P29, P29 + 1), (0, P29 - 1, P29 + 1),
           (0, P29 - 100000, P29 - 99000), (0, P29 - 200000, P29 + 400000), (0, P29 + 16384, P29 + 32768), (0, P29 + 100000, P29 + 100500), (0, P29 + 399000, P29 + 400300),
           (0, P29 + 500000, P29 + 500001), (0, P29 + (1 << 26), P29 + (1 << 26) + 5), (0, P30 - 1, P30), (0, P30, P30 + 1), (0, P30 - 1, P30 + 1), (0, P30 - 300000, P30 - 299000),
           (0, P30 - 50000, P30 + 50000), (0, P30 + 16384 * 3, P30 + 16384 * 4), (0, P30 + 299000, P30 + 300300), (0, P30 + 700000, P30 + 700001), (0, P30 + 450000, P30 + 450010),
           (0, cc.TOP - 200000, cc.TOP), (0, cc.TOP - 1, cc.TOP), (0, cc.TOP - 100000, cc.TOP - 99000), (0, 3 << 29, (3 << 29) + 1000), (0, P29, P30), (0, 5000000, P29 - 200000),
           (1, 0, 70000), (1, 0, 1), (1, 16384, 16385), (1, 69999, 70000), (1, 30000, 31000)]


def _query_check(csi_bytes, raw, recs, regions):
    csi, reader, bounds, hits = cc.read_csi(csi_bytes), bc.VReader(raw), [], 0
    for rid, beg, end in regions:
        got = cc.query(csi, reader, rid, beg, end, bounds)
        assert got == bc.brute(recs, rid, beg, end), (rid, beg, end)
        hits += len(got)
    placed = sum(sum(r["meta"][1]) for r in csi["refs"] if r["meta"])
    assert placed + csi["n_no_coor"] == len(recs)
    return csi, hits, bounds


def _is_bgzf_with_eof(raw):
    blocks = bgzfio.split(raw)
    assert raw.endswith(bgzfio.EOF_BLOCK) and len(blocks) >= 2 and blocks[-1]["isize"] == 0
    assert all(0 < b["isize"] <= bgzfio.BLOCK_IN for b in blocks[:-1])
    return bgzfio.inflate(raw)


def test_files_of_both_sinks_indexed_in_one_slab_and_block_by_block(layout):
    ref, d, _ = layout
    recs = _record_set()
    for device in (False, True):
        p = os.path.join(d, "csi_set_%d.bam" % device)
        w = api.BamWriter(p, NAMES, LENS, extra_header="@PG\tID:t\n", threads=2, level=1, device=ref if device else None, coordinate=True)
        for a in range(0, len(recs), 900):
            w.write_encoded(b"".join(recs[a:a + 900]), len(recs[a:a + 900]))
        w.close()
        raw = open(p, "rb").read()
        at, isize = _table(raw)
        hdr = rc.header_len(bgzfio.inflate(raw))
        starts = set((hdr + np.concatenate([[0], np.cumsum([len(r) for r in recs])])).tolist())
        assert len(isize) > 4 and sum(int(c) not in starts for c in np.cumsum(isize)[:-2]) >= 3                  # blocks end inside records
        want = cc.csi_of(recs, hdr, LENS, at, isize, 14)
        for max_bytes, csi_path in ((0, None), (1, p + ".blockwise.csi")):
            st = api.bam_index_csi(p, csi_path, max_bytes=max_bytes, timed=bool(max_bytes))
            print("device writer" if device else "host writer", max_bytes, st)
            target = csi_path or p + ".csi"
            assert _is_bgzf_with_eof(open(target, "rb").read()) == want, (device, max_bytes)
            assert (st["min_shift"], st["depth"]) == (14, 6) and st["records"] == len(recs) and st["blocks"] == len(isize) and st["n_no_coor"] == 41
            assert st["slabs"] == 1 if max_bytes == 0 else st["slabs"] >= sum(1 for s in isize if s)
            assert not os.path.exists(target + ".tmp")
        csi, hits, bounds = _query_check(want, raw, recs, REGIONS)
        assert len(REGIONS) >= 30 and hits > len(recs) and sum(1 for b in bounds if b > 0) >= 20
        assert max(max(r["bins"]) for r in csi["refs"]) > 65535 + 37449                                          # leaf bins that 16 bits do not hold
        other = os.path.join(d, "csi_shift_12.csi")                                                              # another min_shift: depth 7
        st = api.bam_index_csi(p, other, min_shift=12)
        assert (st["min_shift"], st["depth"]) == (12, 7) and _is_bgzf_with_eof(open(other, "rb").read()) == cc.csi_of(recs, hdr, LENS, at, isize, 12)


def test_an_index_of_more_than_one_bgzf_block(layout):
    ref, d, _ = layout
    recs = [bc.m(0, P30 + 20000 * k, b"r%d" % k) for k in range(3000)]                  # a leaf bin each: 32 bytes of index a record
    p = os.path.join(d, "csi_many_bins.bam")
    w = api.BamWriter(p, ["big"], [cc.TOP], threads=2, level=1, coordinate=True)
    w.write_encoded(b"".join(recs), len(recs))
    w.close()
    st = api.bam_index_csi(p)
    raw, index = open(p, "rb").read(), open(p + ".csi", "rb").read()
    at, isize = _table(raw)
    assert [b["isize"] for b in bgzfio.split(index)][:-1] == [bgzfio.BLOCK_IN, 20 + 4 + 3000 * 32 + 48 + 8 - bgzfio.BLOCK_IN] and st["bins"] == 3000
    assert _is_bgzf_with_eof(index) == cc.csi_of(recs, rc.header_len(bgzfio.inflate(raw)), [cc.TOP], at, isize, 14)


# ---- 3. finalize
def test_finalize_writes_the_index_that_was_asked_for(layout):
    ref, d, out = layout
    names, offs, clens, alt, l_pac = ref.contigs()
    with pytest.raises(ValueError):
        e2e.finalize(ref, out, os.path.join(d, "never.bam"), chunk=fc.CHUNK, bam_threads=2, index="nonsense")
    assert not os.path.exists(os.path.join(d, "never.bam"))
    fin = {}
    for index in (True, "bai", "auto", "csi"):
        p = os.path.join(d, "fin_%s.bam" % index)
        fin[index] = e2e.finalize(ref, out, p, chunk=fc.CHUNK, bam_threads=2, index=index)
        assert fin[index]["index"]["records"] == fin[index]["records"] > 0 and fin[index]["index_seconds"] > 0
        assert os.path.exists(p + ".csi") == (index == "csi") and os.path.exists(p + ".bai") == (index != "csi")
    assert "index_format" not in fin[True] and [fin[k]["index_format"] for k in ("bai", "auto", "csi")] == ["bai", "bai", "csi"]       # no contig above 2^29 here
    bai = open(os.path.join(d, "fin_True.bam.bai"), "rb").read()
    assert bai == open(os.path.join(d, "fin_auto.bam.bai"), "rb").read() == open(os.path.join(d, "fin_bai.bam.bai"), "rb").read()
    p = os.path.join(d, "fin_csi.bam")
    raw, recs = open(p, "rb").read(), fc.records_of(p)
    assert rc.inflate(p) == rc.inflate(os.path.join(d, "fin_True.bam"))                  # whatever index is asked for, the file's content is the same
    at, isize = _table(raw)
    got = _is_bgzf_with_eof(open(p + ".csi", "rb").read())
    assert got == cc.csi_of(recs, rc.header_len(bgzfio.inflate(raw)), clens, at, isize, 14) and fin["csi"]["index"]["depth"] == 5
    cc.same_as_bai(got, bai)
    regions = [q for i, l in enumerate(clens) for q in ((i, 0, l), (i, l // 2, l // 2 + 1), (i, l - 1, l), (i, max(0, min(l, 16384) - 1), min(l, 16385)))]
    _query_check(got, raw, recs, regions)


# ---- 4. the long contig
def test_the_bai_refuses_the_long_contig_and_names_the_csi(layout):
    ref, d, _ = layout
    p = os.path.join(d, "long.csi.bam")
    w = api.BamWriter(p, ["big"], [(1 << 29) + 1], threads=1, coordinate=True)
    recs = [bc.m(0, 5, b"a"), bc.m(0, 1 << 29, b"last", "1M")]
    w.write_encoded(b"".join(recs), len(recs))
    w.close()
    with pytest.raises(api.ArachneError) as e:
        api.bam_index(p)
    assert e.value.code == api.ARX_E_ARG and "CSI" in str(e.value) and "arx_bam_index_csi" in str(e.value)
    assert not os.path.exists(p + ".bai") and not os.path.exists(p + ".bai.tmp")
    st = api.bam_index_csi(p)
    assert (st["depth"], st["min_shift"], st["records"]) == (6, 14, 2) and os.path.exists(p + ".csi") and not os.path.exists(p + ".csi.tmp")
    raw = open(p, "rb").read()
    at, isize = _table(raw)
    assert _is_bgzf_with_eof(open(p + ".csi", "rb").read()) == cc.csi_of(recs, rc.header_len(bgzfio.inflate(raw)), [(1 << 29) + 1], at, isize, 14)
    for bad in (9, 25, -1):
        with pytest.raises(api.ArachneError) as e:
            api.bam_index_csi(p, p + ".bad.csi", min_shift=bad)
        assert e.value.code == api.ARX_E_ARG and not os.path.exists(p + ".bad.csi")
    with pytest.raises(api.ArachneError) as e:
        api.bam_index_csi(p, device=4096)
    assert e.value.code == api.ARX_E_DEVICE

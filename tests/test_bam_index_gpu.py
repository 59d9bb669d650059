"""The .bai of a coordinate-sorted BAM file on the GPU (arx_bam_index, arx_selftest_bam_index; arachne_amd/csrc/dev_bamindex.h, hip_bamindex.h).
1. the cases of baicases.py -- the ones tests/test_bam_index_sim.py runs through the host program -- through the kernels, at every segment and
slab size, held byte for byte to baicases.bai_of; 2. real files from both sinks, indexed as one slab and a block per slab, the bytes held to
bai_of over the file's own block table and the index queried by the independent reader; 3. e2e.finalize(index=True); 4. what is refused."""
import os
import tempfile

import numpy as np
import pytest

import baicases as bc
import bgzfio
import reccases as rc
import recfullcases as fc
import test_bam_reference_layout as trl
from arachne_amd import api, e2e, synth

pytestmark = pytest.mark.gpu


# ---- 1. the kernels on streams with a block table
@pytest.mark.parametrize("seg", bc.SEGS)
def test_cases_through_the_kernels(seg):
    for name, case in bc.cases().items():
        for slab in case.slabs:
            code, bai, st = api.selftest_bam_index(case.stream, case.hdr, case.ref_len, case.at, case.isize, seg, slab)
            if case.refused is None:
                assert code == 0 and bai == case.want, (name, slab)
                assert st["records"] == len(case.recs) and st["n_no_coor"] == bc.read_bai(bai)["n_no_coor"], (name, slab)
            else:
                assert code == case.refused.code and bai == b"", (name, slab)
                if case.refused.record is not None:
                    assert (st["refused"] >> 8, st["refused"] & 0xff) == (case.refused.record, case.refused.rule), (name, slab)
        if name.startswith("slab_cuts") or name in ("one_byte_blocks", "longer_than_a_slab"):
            assert api.selftest_bam_index(case.stream, case.hdr, case.ref_len, case.at, case.isize, seg, case.slabs[0])[2]["slabs"] >= 2


@pytest.mark.parametrize("seg", bc.SEGS)
def test_broken_chains_are_refused(seg):
    for name, case in bc.broken().items():
        for slab in case.slabs:
            code, bai, st = api.selftest_bam_index(case.stream, case.hdr, case.ref_len, case.at, case.isize, seg, slab)
            assert code == api.ARX_E_IO and bai == b"", (name, slab)


def test_bad_arguments_and_a_small_buffer():
    case = bc.cases()["one_record"]
    assert api.selftest_bam_index(case.stream, case.hdr, case.ref_len, case.at, case.isize, 96)[0] == api.ARX_E_ARG                    # no power of two
    assert api.selftest_bam_index(case.stream, case.hdr, case.ref_len, case.at, case.isize[:-1] + [5], 64)[0] == api.ARX_E_ARG         # sizes that do not sum up
    assert api.selftest_bam_index(case.stream, case.hdr, case.ref_len, [a + (1 << 48) for a in case.at], case.isize, 64)[0] == api.ARX_E_ARG
    code, bai, st = api.selftest_bam_index(case.stream, case.hdr, case.ref_len, case.at, case.isize, 64, out_cap=len(case.want) - 1)
    assert code == api.ARX_E_TOO_LARGE and bai == b""
    assert api.selftest_bam_index(case.stream, case.hdr, case.ref_len, case.at, case.isize, 64, out_cap=len(case.want))[1] == case.want


# ---- 2. and 3. files
NAMES, LENS = ["chrA", "chrB", "chrEmpty", "chrC"], [400000, 150000, 70000, 3000]


def _record_set():
    """a few thousand sorted records on three of four contigs, read lengths mixed so that the writers' blocks end inside records"""
    rng = np.random.default_rng(11)
    recs = []
    for rid, n in ((0, 2200), (1, 900), (3, 150)):
        for k, pos in enumerate(sorted(int(x) for x in rng.integers(0, LENS[rid] - 600, n))):
            l = int(rng.integers(30, 260))
            kind = k % 9
            if kind == 0:
                recs.append(bc.rec(rid, pos, b"u%d_%d" % (rid, k), l_seq=l, flag=4 | 1))                                  # placed with its mate
            elif kind == 1:
                recs.append(bc.m(rid, pos, b"d%d_%d" % (rid, k), "%dS%dM%dD%dM" % (5, l - 25, 3 + k % 300, 20), l_seq=l))
            elif kind == 2 and rid == 0 and pos < 250000:
                recs.append(bc.m(rid, pos, b"n%d_%d" % (rid, k), "%dM%dN%dM" % (10, 20000 + 37 * k, l - 10), l_seq=l))    # spliced across windows and bins
            else:
                recs.append(bc.m(rid, pos, b"m%d_%d" % (rid, k), "%dM" % l, l_seq=l))
    recs += [bc.rec(-1, -1, b"x%d" % k, l_seq=int(rng.integers(20, 200)), flag=4) for k in range(77)]
    keys = [(bc.fields(r)[1] & 0xFFFFFFFF, bc.fields(r)[2]) for r in recs]
    assert keys == sorted(keys) and all(bc.interval(r)[1] <= LENS[bc.fields(r)[1]] for r in recs[:-77])
    return recs


@pytest.fixture(scope="module")
def layout():
    """the reference-layout directory of tests/test_bam_sort_gpu.py's end-to-end test -> (ref, its directory, the layout directory)"""
    g, rs = trl._reads(5, 60)
    d = tempfile.mkdtemp(prefix="arx_bai_")
    fa = rc.make_index(d, g, api.LIB_PATH)
    f1, f2 = os.path.join(d, "a1.fq"), os.path.join(d, "a2.fq")
    synth.write_fastq_fast(rs, f1, f2)
    ref = api.Reference(fa)
    out = os.path.join(d, "out")
    e2e.run(ref, [(f1, f2)], out, pairs_per_batch=70, bam_threads=2, rec_threads=3, layout="reference", chunk=fc.CHUNK)
    yield ref, d, out
    ref.close()


def _table(raw):
    blocks = bgzfio.split(raw)
    return [b["at"] for b in blocks] + [len(raw)], [b["isize"] for b in blocks]


def _query_check(bai_bytes, raw, recs, lens, regions):
    bai = bc.read_bai(bai_bytes)
    hits = 0
    for rid, beg, end in regions:
        got = bc.query(bai, raw, rid, beg, end)
        assert got == bc.brute(recs, rid, beg, end), (rid, beg, end)
        hits += len(got)
    placed = sum(sum(r["pseudo"][1]) for r in bai["refs"] if r["pseudo"])
    assert placed + bai["n_no_coor"] == len(recs)
    return bai, hits


REGIONS = [(0, 0, 400000), (0, 0, 1), (0, 16383, 16384), (0, 16384, 16385), (0, 16383, 16385), (0, 16384 * 3, 16384 * 4), (0, (1 << 17) - 1, (1 << 17) + 1), (0, 1 << 17, (1 << 17) + 50),
           (0, 131000, 132000), (0, 262144 - 10, 262144 + 10), (0, 399000, 400000), (0, 399999, 400000), (0, 100000, 300000), (0, 12345, 12346), (0, 50000, 50500),
           (1, 0, 150000), (1, 0, 16384), (1, 16384, 32768), (1, 149000, 150000), (1, 131072, 131073), (1, 70000, 70001), (1, 1, 2), (2, 0, 70000), (2, 16384, 16385),
           (3, 0, 3000), (3, 0, 1), (3, 2999, 3000), (3, 1000, 2000), (3, 2400, 2401), (0, 65536, 65537)]


def test_files_of_both_sinks_indexed_in_one_slab_and_block_by_block(layout):
    ref, d, _ = layout
    recs = _record_set()
    for device in (False, True):
        p = os.path.join(d, "set_%d.bam" % device)
        w = api.BamWriter(p, NAMES, LENS, extra_header="@PG\tID:t\n", threads=2, level=1, device=ref if device else None, coordinate=True)
        for a in range(0, len(recs), 900):
            w.write_encoded(b"".join(recs[a:a + 900]), len(recs[a:a + 900]))
        w.close()
        raw = open(p, "rb").read()
        at, isize = _table(raw)
        data = bgzfio.inflate(raw)
        hdr = rc.header_len(data)
        starts = set((hdr + np.concatenate([[0], np.cumsum([len(r) for r in recs])])).tolist())
        assert len(isize) > 8 and sum(int(c) not in starts for c in np.cumsum(isize)[:-2]) >= 5                  # blocks end inside records
        want = bc.bai_of(recs, hdr, LENS, at, isize)
        for max_bytes, bai_path in ((0, None), (1, p + ".blockwise.bai")):
            st = api.bam_index(p, bai_path, max_bytes=max_bytes, timed=bool(max_bytes))
            print("device writer" if device else "host writer", max_bytes, st)
            got = open(bai_path or p + ".bai", "rb").read()
            assert got == want, (device, max_bytes)
            assert st["records"] == len(recs) and st["blocks"] == len(isize) and st["n_no_coor"] == 77 and (st["slabs"] == 1 if max_bytes == 0 else st["slabs"] >= sum(1 for s in isize if s))
            assert not os.path.exists((bai_path or p + ".bai") + ".tmp")
        bai, hits = _query_check(want, raw, recs, LENS, REGIONS)
        assert len(REGIONS) >= 30 and hits > len(recs) and bai["refs"][2] == dict(bins={}, pseudo=None, lin=[])


def test_finalize_writes_the_index_beside_the_final_file(layout):
    ref, d, out = layout
    names, offs, clens, alt, l_pac = ref.contigs()
    plain = e2e.finalize(ref, out, os.path.join(d, "final_plain.bam"), chunk=fc.CHUNK, bam_threads=2)
    assert sorted(plain) == ["buckets", "bytes", "records", "seconds", "sort"] and not os.path.exists(os.path.join(d, "final_plain.bam.bai"))
    for sink in ("host", "device"):
        p = os.path.join(d, "final_%s.bam" % sink)
        fin = e2e.finalize(ref, out, p, sink=sink, chunk=fc.CHUNK, bam_threads=2, index=True)
        assert sorted(fin) == sorted(list(plain) + ["index", "index_seconds"])
        assert {k: fin[k] for k in ("records", "buckets")} == {k: plain[k] for k in ("records", "buckets")}
        assert os.path.exists(p + ".bai") and fin["index"]["records"] == fin["records"] > 0
        raw, recs = open(p, "rb").read(), fc.records_of(p)
        got = open(p + ".bai", "rb").read()
        at, isize = _table(raw)
        assert got == bc.bai_of(recs, rc.header_len(bgzfio.inflate(raw)), clens, at, isize)
        regions = [q for i, l in enumerate(clens) for q in ((i, 0, l), (i, l // 2, l // 2 + 1), (i, l - 1, l), (i, max(0, min(l, 16384) - 1), min(l, 16385)))]
        _query_check(got, raw, recs, clens, regions)
    assert rc.inflate(os.path.join(d, "final_plain.bam")) == rc.inflate(os.path.join(d, "final_host.bam"))                  # index=True leaves the file's content alone


def _refused(path, code, bai_path=None, **kw):
    target = bai_path or path + ".bai"
    with pytest.raises(api.ArachneError) as e:
        api.bam_index(path, bai_path, **kw)
    assert e.value.code == code, str(e.value)
    assert not os.path.exists(target) and not os.path.exists(target + ".tmp")
    return str(e.value)


def test_what_is_refused(layout):
    ref, d, _ = layout
    recs = _record_set()
    foreign = os.path.join(d, "foreign.bam")
    w = api.BamWriter(foreign, NAMES, LENS, threads=1, level=1)
    mixed = recs[:2000] + recs[100:200] + recs[2000:]                                    # not sorted: record 2000 is the first offender
    w.write_encoded(b"".join(mixed), len(mixed))
    w.close()
    for max_bytes in (0, 1):
        text = _refused(foreign, api.ARX_E_ARG, max_bytes=max_bytes)
        assert "record 2000" in text and "sorted" in text
    good = os.path.join(d, "good.bam")
    w = api.BamWriter(good, NAMES, LENS, threads=1, level=1)
    w.write_encoded(b"".join(recs), len(recs))
    w.close()
    raw = open(good, "rb").read()
    cut = os.path.join(d, "cut.bam")
    with open(cut, "wb") as f:
        f.write(raw[:len(raw) // 2])                                                     # ends inside a BGZF block
    _refused(cut, api.ARX_E_IO)
    chain = os.path.join(d, "chain.bam")
    bgzfio.write_bgzf_file(chain, bgzfio.inflate(raw)[:-7])                              # the last record runs past the end
    _refused(chain, api.ARX_E_IO)
    _refused(chain, api.ARX_E_IO, max_bytes=1)
    _refused(os.path.join(d, "no_such_file.bam"), api.ARX_E_IO)
    _refused(good, api.ARX_E_IO, bai_path=os.path.join(d, "no_such_directory", "x.bai"))
    long_contig = os.path.join(d, "long.bam")
    api.BamWriter(long_contig, ["big"], [(1 << 29) + 1], threads=1).close()
    assert "CSI" in _refused(long_contig, api.ARX_E_ARG)
    with pytest.raises(api.ArachneError) as e:
        api.bam_index(good, device=4096)
    assert e.value.code == api.ARX_E_DEVICE and not os.path.exists(good + ".bai")
    assert api.bam_index(good)["records"] == len(recs) and os.path.exists(good + ".bai")                  # and the good file is accepted

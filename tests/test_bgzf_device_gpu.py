"""The device BAM sink on the GPU (arx_bam_open_device, arx_selftest_bgzf; arachne_amd/csrc/dev_bgzf.h, hip_bgzf.h): BGZF blocks deflated and
checksummed by HIP kernels.  The pin is the one of test_bam_sink.py: after inflating every block with Python's zlib the stream is byte for
byte what the host sink's file inflates to, and the framing is valid (bgzfcases.py: magic, BC subfield, BSIZE, CRC-32, ISIZE, the cut at
multiples of 65280).  Compressed bytes may differ from zlib's; they may not differ between two runs, batch sizes or thread counts."""
import os
import tempfile
import zlib

import numpy as np
import pytest

import bgzfcases
from arachne_amd import api, e2e, synth

pytestmark = pytest.mark.gpu
CONTIGS, CONTIG_LENS = ["chrA", "chrB_random", "c3"], [600000000, 1234567, 88]


@pytest.fixture(scope="module")
def ref():
    g = synth.make_genome(15, [400000, 150000])
    d = tempfile.mkdtemp(prefix="arx_bgzf_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    api.index_build(fa, fa)
    r = api.Reference(fa)
    r.genome, r.dir = g, d
    yield r
    r.close()


# ---- 1. edge inputs through the self-test entry
@pytest.fixture(scope="module")
def cases():
    return bgzfcases.edge_inputs()


@pytest.mark.parametrize("name", sorted(bgzfcases.edge_inputs()))
def test_edge_input(cases, name):
    raw, forms = api.bgzf_selftest(cases[name])
    print(name, len(cases[name]), "->", len(raw), forms)
    bgzfcases.check_case(name, cases[name], raw, forms)
    if name == "e_distance_32769":
        assert len(raw) >= 65280    # nothing to gain inside the window; a match at distance 32769 would have failed to inflate above


def test_no_input_no_block():
    raw, forms = api.bgzf_selftest(b"")
    assert raw == b"" and forms == dict(blocks=0, stored=0, fixed=0, dynamic=0)


def test_selftest_is_deterministic_and_independent_of_the_neighbours(cases):
    a, b = cases["a_text_130561"], cases["h_fibonacci"]
    one = api.bgzf_selftest(a)[0]
    assert api.bgzf_selftest(a)[0] == one
    # the first block of a, alone and in front of other blocks: the same bytes
    first = api.bgzf_selftest(a[:65280])[0]
    assert one.startswith(first) and api.bgzf_selftest(a[:65280] + b)[0].startswith(first)


# ---- 1b. more than two groups of 256 blocks through one flush: both staging pairs are reused, groups reach the sink in order
def _varying(n, seed):
    """n compressible bytes whose content changes along the stream: eight values around a level that moves every 4099 bytes, so that no two
    blocks, and no two groups, look alike -- a block written twice, dropped or out of order cannot inflate to the input"""
    rng = np.random.default_rng(seed)
    pos = np.arange(n, dtype=np.int64)
    return ((rng.integers(0, 8, n, dtype=np.uint8) + (pos // 4099 * 37 % 241)).astype(np.uint8) ^ (pos // 65280 % 251).astype(np.uint8)).tobytes()


def test_many_groups_through_one_flush():
    data = _varying(600 * 65280 + 12345, 11)        # 601 blocks: groups of 256, 256 and 89 -- the first staging pair is used a second time
    raw, forms = api.bgzf_selftest(data)
    sizes = bgzfcases.check_stream(raw, data)
    assert len(sizes) == 601 == forms["blocks"] and forms["stored"] == 0
    assert len(raw) < 0.9 * len(data)     # at most 17 levels x 8 values in a block: log2(136) = 7.1 bits a byte with a Huffman code alone


def test_device_writer_one_large_write_against_host_writer(ref, tmp_path):
    n = 120_000                                       # about 36 MB in one arx_bam_write: three groups in one flush of the writer
    rng = np.random.default_rng(12)
    names = np.frombuffer(b"".join(b"q%08d" % i for i in range(n)), dtype=np.uint8)
    name_off = np.arange(n + 1, dtype=np.int64) * 9
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, 150), dtype=np.uint8)]
    qual = (np.array([2, 12, 23, 37], np.uint8)[rng.integers(0, 4, size=(n, 150), dtype=np.uint8)] + 33).astype(np.uint8)
    aux1 = b"RGZlib1\0ASC\x96XMZ0\0BXZA01C02B03D04-1\0"
    aux = np.frombuffer(aux1 * n, dtype=np.uint8)
    flag = np.full(n, 99, np.int32); rid = np.zeros(n, np.int32); pos = rng.integers(0, 500_000_000, size=n).astype(np.int32); mapq = np.full(n, 60, np.uint8)
    mrid = np.zeros(n, np.int32); mpos = pos + 200; tlen = np.full(n, 350, np.int32)
    cig_off = np.arange(n + 1, dtype=np.int64); cig = np.full(n, 150 << 4, np.uint32)
    seq_off = np.arange(n + 1, dtype=np.int64) * 150
    aux_off = np.arange(n + 1, dtype=np.int64) * len(aux1)
    view = api._BamBatch(n, name_off.ctypes.data, names.ctypes.data, flag.ctypes.data, rid.ctypes.data, pos.ctypes.data, mapq.ctypes.data, mrid.ctypes.data, mpos.ctypes.data,
                         tlen.ctypes.data, cig_off.ctypes.data, cig.ctypes.data, seq_off.ctypes.data, seq.ctypes.data, qual.ctypes.data, 33, aux_off.ctypes.data, aux.ctypes.data)
    got = {}
    for dev, f in ((None, "h.bam"), (ref, "d.bam")):
        w = api.BamWriter(str(tmp_path / f), CONTIGS, CONTIG_LENS, threads=8, level=1, device=dev)
        w.write_view(view)
        st = w.close()
        got[f] = (st, _inflated(str(tmp_path / f))[1])
    (sh, bh), (sd, bd) = got["h.bam"], got["d.bam"]
    assert len(bh) > 2 * 256 + 1 and bd == bh                      # the same cuts, the same bytes, the same order
    assert (sd["records"], sd["blocks"], sd["bytes_in"]) == (sh["records"], sh["blocks"], sh["bytes_in"]) == (n, len(bh), sum(len(b) for b in bh))


# ---- 2. device writer against host writer (the record generator of test_bam_sink.py)
def _records(n, rng, names_c):
    recs = []
    for i in range(n):
        l_seq = int(rng.integers(0, 200)) if i % 17 else 0
        unm = i % 11 == 0
        ops = [(int(rng.integers(0, 9)), int(rng.integers(1, 90))) for _ in range(int(rng.integers(0, 6)))] if not unm else []
        cig = np.array([l << 4 | op for op, l in ops], dtype=np.uint32)
        name = ("r%d:%s" % (i, "x" * int(rng.integers(0, 40)))).encode()
        seq = bytes(rng.choice(list(b"ACGTNacgtn=MRSVWYHKDB"), size=l_seq).astype(np.uint8))
        qual = bytes((rng.integers(0, 42, size=l_seq) + 33).astype(np.uint8))
        aux = b"ASC" + bytes([int(rng.integers(0, 150))]) + b"BXZ" + ("A%02dC%02d-1" % (i % 96, i % 7)).encode() + b"\0" if i % 3 else b""
        recs.append(dict(name=name, flag=int(rng.integers(0, 4096)), rid=-1 if unm else int(rng.integers(0, names_c)), pos=-1 if unm else int(rng.integers(0, 2 ** 29 - 5000)),
                         mapq=int(rng.integers(0, 61)), mate_rid=int(rng.integers(-1, names_c)), mate_pos=int(rng.integers(-1, 1000000)), tlen=int(rng.integers(-900, 900)),
                         cigar=cig, seq=seq, qual=qual, aux=aux))
    return recs


def _write(path, recs, threads, batch, device=None):
    w = api.BamWriter(path, CONTIGS, CONTIG_LENS, extra_header="@RG\tID:lib1\tSM:s\n@PG\tID:arachne_amd\n", threads=threads, device=device)
    for o in range(0, len(recs), batch):
        part = recs[o:o + batch]
        w.write([r["name"] for r in part], [r["flag"] for r in part], [r["rid"] for r in part], [r["pos"] for r in part], [r["mapq"] for r in part],
                [r["mate_rid"] for r in part], [r["mate_pos"] for r in part], [r["tlen"] for r in part], [r["cigar"] for r in part],
                [r["seq"] for r in part], [r["qual"] for r in part], [r["aux"] for r in part])
    return w.close()


def _inflated(path):
    raw = open(path, "rb").read()
    assert raw[-28:] == bgzfcases.EOF_BLOCK
    blocks = [b for b, _ in bgzfcases.bgzf_blocks(raw)]
    assert blocks[-1] == b""
    return raw, blocks[:-1]


def test_device_writer_against_host_writer(ref, tmp_path):
    recs = _records(5000, np.random.default_rng(3), 3)
    ph, p1, p2, p3 = (str(tmp_path / f) for f in ("host.bam", "d700.bam", "d1999.bam", "again.bam"))
    sh = _write(ph, recs, 1, 700)
    s1 = _write(p1, recs, 1, 700, device=ref)
    s2 = _write(p2, recs, 8, 1999, device=ref)
    _write(p3, recs, 3, 700, device=ref)
    raw_h, blocks_h = _inflated(ph)
    raw_1, blocks_1 = _inflated(p1)
    assert blocks_1 == blocks_h                                     # the same cuts, the same bytes
    for s in (s1, s2):
        assert (s["records"], s["blocks"], s["bytes_in"]) == (sh["records"], sh["blocks"], sh["bytes_in"]) == (5000, len(blocks_h), sum(len(b) for b in blocks_h))
    assert s1["bytes_out"] == len(raw_1)
    assert open(p2, "rb").read() == raw_1 and open(p3, "rb").read() == raw_1    # batch size, threads and the run do not change a byte


def test_write_select_device_against_host(ref, tmp_path):
    recs = _records(1500, np.random.default_rng(4), 3)
    n = len(recs)

    def cat(parts, dt=np.uint8):
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(p) for p in parts])
        flat = np.concatenate([np.frombuffer(p, dtype=np.uint8) if isinstance(p, bytes) else np.asarray(p, dtype=dt) for p in parts])
        return off, np.ascontiguousarray(flat, dtype=dt)
    name_off, name_b = cat([r["name"] for r in recs])
    cig_off, cig_w = cat([r["cigar"] for r in recs], np.uint32)
    seq_off, seq_b = cat([r["seq"] for r in recs])
    _q, qual_b = cat([r["qual"] for r in recs])
    aux_off, aux_b = cat([r["aux"] for r in recs])
    col = {k: np.ascontiguousarray([r[k] for r in recs], dtype=dt) for k, dt in (("flag", np.int32), ("rid", np.int32), ("pos", np.int32), ("mapq", np.uint8),
                                                                                 ("mate_rid", np.int32), ("mate_pos", np.int32), ("tlen", np.int32))}
    view = api._BamBatch(n, name_off.ctypes.data, name_b.ctypes.data, col["flag"].ctypes.data, col["rid"].ctypes.data, col["pos"].ctypes.data, col["mapq"].ctypes.data,
                         col["mate_rid"].ctypes.data, col["mate_pos"].ctypes.data, col["tlen"].ctypes.data, cig_off.ctypes.data, cig_w.ctypes.data, seq_off.ctypes.data,
                         seq_b.ctypes.data, qual_b.ctypes.data, 33, aux_off.ctypes.data, aux_b.ctypes.data)
    idx = np.random.default_rng(5).permutation(n)[:1100].astype(np.int64)
    out = []
    for dev, f in ((None, "h.bam"), (ref, "d.bam")):
        w = api.BamWriter(str(tmp_path / f), CONTIGS, CONTIG_LENS, threads=4, device=dev)
        w.write_select(view, idx[:600])
        w.write_select(view, idx[600:])
        st = w.close()
        assert st["records"] == 1100
        out.append(_inflated(str(tmp_path / f))[1])
    assert out[0] == out[1] and sum(len(b) for b in out[0]) > 65280


# ---- 3. it compresses
def test_it_compresses(cases):
    data = bgzfcases.bam_like_stream(4000)
    raw, forms = api.bgzf_selftest(data)
    bgzfcases.check_stream(raw, data)
    fixed, huff, plain = (bgzfcases.zlib_size(data, s) for s in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_DEFAULT_STRATEGY))
    print("ratios: device %.3f, zlib level 1 %.3f, Z_FIXED %.3f, Z_HUFFMAN_ONLY %.3f" % tuple(len(data) / x for x in (len(raw), plain, fixed, huff)))
    assert len(raw) < fixed and len(raw) < huff
    assert forms["stored"] == 0 and forms["blocks"] == (len(data) + 65279) // 65280


# ---- 4. end to end
@pytest.mark.parametrize("layout", ["workers", "reference"])
def test_end_to_end_device_sink_against_host_sink(ref, layout):
    rs = synth.make_reads(16, ref.genome, 20, 100, invalid_frac=0.25)
    assert rs.n_pairs == 2000
    d = tempfile.mkdtemp(prefix="arx_bgzf_e2e_", dir=ref.dir)
    f1, f2 = os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq")
    synth.write_fastq_fast(rs, f1, f2, 0, rs.n_pairs)
    outs = {}
    for sink in ("host", "device"):
        out = os.path.join(d, "out_" + sink)
        st = e2e.run(ref, [(f1, f2)], out, pairs_per_batch=700, bam_threads=2, rec_threads=3, layout=layout, chunk=100000, sink=sink)
        assert st["pairs"] == 2000
        files = {f: os.path.join(out, f) for f in st["files"]} if layout == "reference" else {"0.bam": out + ".0.bam"}
        outs[sink] = {name: _inflated(f)[1] for name, f in files.items()}
    assert outs["host"].keys() == outs["device"].keys() and (len(outs["host"]) == 1 if layout == "workers" else len(outs["host"]) > 2)
    for f in outs["host"]:
        assert outs["device"][f] == outs["host"][f], f
    assert max(sum(len(b) for b in blocks) for blocks in outs["host"].values()) > 65280     # whole blocks went through the kernels, not only last ones


# ---- 5. errors
def test_errors(ref, tmp_path):
    import ctypes as C
    with pytest.raises(api.ArachneError, match="cannot write"):
        api.BamWriter(str(tmp_path / "no_such_dir" / "x.bam"), ["c"], [10], device=ref)
    fn = api._selftest_fn(ref.lib, "arx_bam_open_device")
    h, msg = C.c_void_p(), C.create_string_buffer(256)
    names = (C.c_char_p * 1)(b"c")
    lens = np.array([10], np.int32)
    assert fn(None, str(tmp_path / "y.bam").encode(), 1, names, lens.ctypes.data, None, 1, C.byref(h), msg, 256) == -2    # ARX_E_ARG
    assert not h.value and b"context" in msg.value
    assert fn(ref.h, str(tmp_path / "no_such_dir" / "x.bam").encode(), 1, names, lens.ctypes.data, None, 1, C.byref(h), msg, 256) == -5   # ARX_E_IO
    assert not h.value and msg.value

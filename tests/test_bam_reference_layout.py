"""The reference's output layout (CreateBAMs / AppendBams / AppendBam, bamwriter.go:127-190, 278-566, 635-689): e2e.run(layout="reference")
writes bc_sorted_bam.bam, the position buckets and ZZZ_unmapped_pos_bucketed.bam, every record twice, with split records and the full tag set.

Every file is read back with the BAM reader below and compared with a Python restatement of DoDumpToBam -> AppendBams -> AppendBam that
keeps the reference's in-place mutation (pos = -1, mapq = 0 on an alignment the score rule unmaps, seen by every record written after it),
built from the candidate records, post-pass lists and tags of a second run over the same reads (the _expected pattern of test_e2e.py).
Unit tests cover the bucket table and arx_bam_write_select.  GPU variant: tests marked gpu."""
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

from arachne_amd import api, e2e, synth

HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "hostsim", "libarx_hostsim.so")
CODE = "=ACMGRSVTWYHKDBN"


@pytest.fixture(scope="module")
def sim(built):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    return SIM


def _read_bam(path):
    raw = open(path, "rb").read()
    data, o = b"", 0
    while o < len(raw):
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        data += zlib.decompress(raw[o + 18:o + bsize - 8], -15)
        o += bsize
    l_text = struct.unpack_from("<i", data, 4)[0]
    text = data[8:8 + l_text].decode()
    o = 8 + l_text
    n_ref = struct.unpack_from("<i", data, o)[0]; o += 4
    for _ in range(n_ref):
        l = struct.unpack_from("<i", data, o)[0]; o += 4 + l + 4
    recs = []
    while o < len(data):
        bs = struct.unpack_from("<i", data, o)[0]
        rid, pos, l_name, mapq, bn, n_cig, flag, l_seq, mrid, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", data, o + 4)
        q = o + 36
        name = data[q:q + l_name - 1].decode(); q += l_name
        cig = [int(x) for x in np.frombuffer(data, dtype="<u4", count=n_cig, offset=q)]; q += 4 * n_cig
        packed = data[q:q + (l_seq + 1) // 2]; q += (l_seq + 1) // 2
        seq = "".join(CODE[b >> 4] + CODE[b & 15] for b in packed)[:l_seq]
        qual = data[q:q + l_seq]; q += l_seq
        recs.append(dict(name=name, rid=rid, pos=pos, mapq=mapq, flag=flag, mrid=mrid, mpos=mpos, tlen=tlen, cigar=cig, seq=seq, qual=qual,
                         aux=data[q:o + 4 + bs], raw=data[o:o + 4 + bs]))
        o += 4 + bs
    return text, recs


# ---- the bucket table and the selective write
def test_bucket_table_packing_rule(sim):
    """CreateBAMs (bamwriter.go:134-188) with chunk 40 kb: the 50 kb and 120 kb contigs get 2 and 3 files; the 1 kb contig opens a packed
    file, and the 2 kb contig after the 120 kb one joins it (a multi-chunk contig does not reset running_size)."""
    t = api.bucket_table(["a", "b", "c", "d"], [50000, 1000, 120000, 2000], 40000, lib_path=sim)
    assert t.files == ["000000-a_0000000000_pos_bucketed.bam", "000000-a_0000040000_pos_bucketed.bam", "000001-b_0000000000_pos_bucketed.bam",
                       "000002-c_0000000000_pos_bucketed.bam", "000002-c_0000040000_pos_bucketed.bam", "000002-c_0000080000_pos_bucketed.bam",
                       "ZZZ_unmapped_pos_bucketed.bam"]
    assert list(t.contig_file[:4]) == [0, 2, 3, 2]
    t = api.bucket_table(["a", "b", "c"], [30000, 10000, 1], 40000, lib_path=sim)   # 30000 + 10000 <= 40000 packs, + 1 does not
    assert t.files == ["000000-a_0000000000_pos_bucketed.bam", "000002-c_0000000000_pos_bucketed.bam", "ZZZ_unmapped_pos_bucketed.bam"]
    assert list(t.contig_file[:3]) == [0, 0, 1]


def _hand_records(n):
    rng = np.random.default_rng(4)
    names = [b"q%d" % i for i in range(n)]
    seqs = [bytes(rng.choice(list(b"ACGTN"), size=int(rng.integers(1, 40)))) for _ in range(n)]
    quals = [bytes(rng.integers(33, 74, size=len(s), dtype=np.uint8)) for s in seqs]
    cig = [np.array([(len(s) << 4) | 0], dtype=np.uint32) for s in seqs]
    aux = [b"XSi" + struct.pack("<i", -i) + b"XCZ" + b"1,2,1;" * i + b"\0" for i in range(n)]
    ints = [rng.integers(0, 1000, size=n) for _ in range(3)]
    return dict(names=names, flag=rng.integers(0, 4096, size=n), rid=np.zeros(n, dtype=np.int32), pos=ints[0], mapq=rng.integers(0, 61, size=n),
                mate_rid=np.zeros(n, dtype=np.int32), mate_pos=ints[1], tlen=ints[2] - 500, cigars=cig, seqs=seqs, quals=quals, aux=aux)


def test_write_select_equals_write_of_the_subset(sim):
    """arx_bam_write_select(view, idx) writes exactly the bytes arx_bam_write writes for a batch of those records in that order"""
    d = tempfile.mkdtemp(prefix="arx_sel_")
    h = _hand_records(7)
    idx = [5, 0, 3, 3]
    a = api.BamWriter(os.path.join(d, "a.bam"), ["c"], [100000], threads=2, lib_path=sim)
    full = _view(h, sim)
    a.write_select(full["view"], np.array(idx))
    a.close()
    b = api.BamWriter(os.path.join(d, "b.bam"), ["c"], [100000], threads=2, lib_path=sim)
    sub = {k: ([v[i] for i in idx] if isinstance(v, list) else np.asarray(v)[idx]) for k, v in h.items()}
    b.write(sub["names"], sub["flag"], sub["rid"], sub["pos"], sub["mapq"], sub["mate_rid"], sub["mate_pos"], sub["tlen"], sub["cigars"], sub["seqs"], sub["quals"], sub["aux"])
    b.close()
    ra, rb = _read_bam(os.path.join(d, "a.bam"))[1], _read_bam(os.path.join(d, "b.bam"))[1]
    assert [r["raw"] for r in ra] == [r["raw"] for r in rb] and len(ra) == 4
    assert [r["name"] for r in ra] == ["q5", "q0", "q3", "q3"]


def _view(h, lib_path):
    """the hand records as an arx_bam_batch view (what RecBuf.build returns), arrays kept alive in the dict"""
    n = len(h["names"])
    keep = {}

    def cat(parts, dt=np.uint8):
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(p) for p in parts])
        flat = np.concatenate([np.frombuffer(p, dtype=np.uint8) if isinstance(p, bytes) else np.asarray(p, dtype=dt) for p in parts])
        return off, np.ascontiguousarray(flat, dtype=dt)
    for k, dt in (("names", np.uint8), ("cigars", np.uint32), ("seqs", np.uint8), ("quals", np.uint8), ("aux", np.uint8)):
        keep[k] = cat(h[k], dt)
    for k, dt in (("flag", np.int32), ("rid", np.int32), ("pos", np.int32), ("mapq", np.uint8), ("mate_rid", np.int32), ("mate_pos", np.int32), ("tlen", np.int32)):
        keep[k] = np.ascontiguousarray(h[k], dtype=dt)
    v = api._BamBatch(n, keep["names"][0].ctypes.data, keep["names"][1].ctypes.data, keep["flag"].ctypes.data, keep["rid"].ctypes.data, keep["pos"].ctypes.data,
                      keep["mapq"].ctypes.data, keep["mate_rid"].ctypes.data, keep["mate_pos"].ctypes.data, keep["tlen"].ctypes.data, keep["cigars"][0].ctypes.data,
                      keep["cigars"][1].ctypes.data, keep["seqs"][0].ctypes.data, keep["seqs"][1].ctypes.data, keep["quals"][1].ctypes.data, 33,
                      keep["aux"][0].ctypes.data, keep["aux"][1].ctypes.data)
    keep["view"] = v
    return keep


# ---- the restatement of DoDumpToBam
class Aln(dict):
    __getattr__ = dict.__getitem__

    def __setattr__(self, k, v):
        self[k] = v


def _is_pair(a, b):
    if a.reversed == b.reversed or a.rid != b.rid:
        return False
    dist = (a.pos - b.pos) if a.reversed else (b.pos - a.pos)
    return -35 <= dist < 750


def _expected(rs, names, table, cands, cand_off, alns, cigars, post, split, mm_ref, mm_read, tags):
    """-> [(bucket, record dict)] in write order; Alignment objects are shared, so AppendBam's mutation is seen by later records"""
    objs = {}

    def aln(i):
        if i not in objs:
            c = cands[i]
            p = post[i]
            cg = []
            if c["reg"] >= 0:
                a = alns[c["reg"]]
                cg = [(int(w) & 15, int(w) >> 4) for w in cigars[a["cigar_off"]:a["cigar_off"] + a["n_cigar"]]]
            objs[i] = Aln(i=i, pos=int(c["pos"]), aend=int(c["aend"]), rid=int(c["rid"]), reversed=bool(c["reversed"]), score=int(c["score"]),
                          is_proper=bool(c["is_proper"]), mapq=int(c["mapq"]), active_molecule=bool(c["active_molecule"]), mol=int(c["molecule_id"]),
                          duplicate=bool(p["duplicate"]), cigar=cg, mm=list(zip(mm_ref[p["mm_off"]:p["mm_off"] + p["n_mm"]], mm_read[p["mm_off"]:p["mm_off"] + p["n_mm"]])),
                          secondary=None, primary=None, mate=None)
        return objs[i]

    po = rs.pair_offsets()
    pair_bc = np.repeat(np.arange(len(po) - 1), np.diff(po))
    act = [int(tags["active"][r]) for r in range(len(rs.lens))]
    for r in range(len(rs.lens)):
        a = aln(act[r])
        a.mate = aln(act[r ^ 1])
        a.read = r
        s = split[r]
        if s["split"] >= 0:
            x = aln(int(s["split"]))
            x.is_proper, x.mapq, x.primary, x.read = bool(s["is_proper"]), int(s["mapq"]), a, r
            a.secondary = x
    dm = {}
    for i in range(len(cands)):
        if cands[i]["active"] and cands[i]["molecule_id"] >= 0:
            k = (int(pair_bc[cands[i]["read"] // 2]), int(cands[i]["molecule_id"]))
            n, sm = dm.get(k, (0, 0))
            dm[k] = (n + 1, sm + int(cands[i]["mismatches"]))

    def zs(tag, s):
        return tag + b"Z" + s + b"\0"

    def ii(tag, v):
        return tag + b"i" + struct.pack("<i", v)

    def mms(x):
        return b"".join(b"%d,%d,1;" % (int(ref), int(rd)) for ref, rd in x.mm)

    def sa(x, hard):
        cg = x.cigar[::-1] if x.reversed else x.cigar
        cs = "".join(f"{ln}{'H' if (op == 3 and hard) else 'MIDS'[op]}" for op, ln in cg)
        nm = len(x.mm) + sum(ln for op, ln in x.cigar if op in (1, 2))
        return f"{names[x.rid]},{x.pos},{'-' if x.reversed else '+'},{cs},{x.mapq},{nm};".encode()

    out = []

    def append(x, primary):
        r = x.read
        p = r // 2
        if not x.is_proper and x.score - 17 < 19:
            x.pos, x.mapq = -1, 0
        fl = 1
        if x.is_proper and (x is primary or _is_pair(x, primary.mate)):
            fl |= 2
        m = primary.mate
        if m.pos == -1 or (not primary.is_proper and m.score - 17 < 19):
            fl |= 8
            mrid, mpos = -1, -1
        else:
            fl |= 0x20 if m.reversed else 0
            mrid, mpos = m.rid, m.pos
        fl |= 0x80 if r & 1 else 0x40
        fl |= 0x400 if x.duplicate else 0
        tl = 0
        if m.pos != -1 and x is primary and x.rid == m.rid and (primary.is_proper or m.score - 17 >= 19):
            tl = -(x.aend - m.pos) if x.reversed else m.aend - x.pos
        if x is not primary:
            fl |= 0x100
        rid, mq = x.rid, x.mapq
        if x.pos == -1:
            fl |= 4
            mq, rid = 0, -1
        fl |= 0x10 if x.reversed else 0
        L = int(rs.lens[r])
        bases = rs.seqs[r][:L]
        seq = "".join("TGCAN"[b] for b in bases[::-1]) if x.reversed else "".join("ACGTN"[b] for b in bases)
        qual = bytes([40] * L)
        cg = [([0, 1, 2, 4, 5][op], ln) for op, ln in x.cigar]
        if x is not primary:                                                    # HardClip (:660-689)
            lo, hi = 0, L
            if len(cg) >= 1 and cg[0][0] == 4:
                lo = cg[0][1]; cg[0] = (5, cg[0][1])
            if len(cg) >= 2 and cg[-1][0] == 4:
                hi -= cg[-1][1]; cg[-1] = (5, cg[-1][1])
            seq, qual = seq[lo:hi], qual[lo:hi]
        t = tags[r]
        aux = zs(b"RG", b"VX:i:1" if rs.valid[p] else b"VX:i:0")
        if x is primary:
            sb = aln(int(t["second_best"])) if t["second_best"] >= 0 else None
            aux += ii(b"XS", int(t["xs"])) + zs(b"XC", mms(sb) if sb else b"") + zs(b"AC", mms(x)) + ii(b"AS", int(t["as"]))
            aux += zs(b"XM", b"1" if (sb and sb.active_molecule) else b"0") + zs(b"AM", b"1" if x.active_molecule else b"0")
            aux += ii(b"XT", 1 if (sb and x.mol == sb.mol) else 0)
        else:
            s = split[r]
            aux += ii(b"XS", int(s["second_best2"] / 2)) + zs(b"XC", b"") + zs(b"AC", mms(x)) + ii(b"AS", int(s["score2"] / 2))
            aux += zs(b"XM", b"0") + zs(b"AM", b"1" if x.active_molecule else b"0") + ii(b"XT", 0)
        other = x.secondary if x.secondary is not None else x.primary
        if other is not None and other.pos > -1:
            aux += zs(b"SA", sa(other, x.secondary is not None))
        bc = rs.barcodes[rs.barcode_id[p]]
        if "-" in bc:
            aux += zs(b"BX", bc.encode()) + ii(b"VX", 1)
            if x is primary and x.active_molecule:
                n, sm = dm[(int(pair_bc[p]), x.mol)]
                aux += zs(b"DM", b"%.6f" % (sm / n))
        unm = not x.is_proper and x.score - 17 < 19                               # IsUnmapped, after the mutation (:280)
        bucket = len(table.files) - 1 if unm else int(table.contig_file[x.rid]) + x.pos // table.chunk
        out.append((bucket, dict(name="r%09d" % p, rid=rid, pos=x.pos, mapq=mq & 255, flag=fl, mrid=mrid, mpos=mpos, tlen=tl,
                                 cigar=[(ln << 4) | op for op, ln in cg], seq=seq, qual=qual, aux=aux)))

    for r in range(len(rs.lens)):
        a = aln(act[r])
        append(a, a)
        if a.secondary is not None:
            append(a.secondary, a)
    return out


def _reads(n_bc, ppb):
    g = synth.make_genome(15, [400000, 150000])
    for s in g.seqs:
        s[s > 3] = 0
    rs = synth.make_reads(16, g, n_bc, ppb, invalid_frac=0.25)
    rs.seqs[5] = np.random.default_rng(1).integers(0, 4, size=150)          # an unmappable read
    rng = np.random.default_rng(8)
    c0 = g.seqs[0]
    for p in rng.choice(np.arange(2, rs.n_pairs), size=max(3, rs.n_pairs // 20), replace=False):
        A = int(rng.integers(1000, 300000))                                   # chimeric R1: 80 bases at A, 70 bases 50 kb away; the mate next to A
        B = A + 50000
        rs.seqs[2 * p] = np.concatenate([c0[A:A + 80], c0[B + 80:B + 150]])
        rs.seqs[2 * p + 1] = (3 - c0[A + 200:A + 350][::-1]).astype(np.uint8)
        rs.lens[2 * p:2 * p + 2] = 150
    return g, rs


def _layout(lib_path, n_bc, ppb, workers, chunk=100000):
    g, rs = _reads(n_bc, ppb)
    d = tempfile.mkdtemp(prefix="arx_layout_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    api.index_build(fa, fa, lib_path=lib_path)
    po = rs.pair_offsets()
    cuts = [int(po[len(po) * k // workers]) for k in range(workers)] + [rs.n_pairs]
    files = []
    for k in range(workers):
        f1, f2 = os.path.join(d, f"r1_{k}.fq"), os.path.join(d, f"r2_{k}.fq")
        synth.write_fastq_fast(rs, f1, f2, cuts[k], cuts[k + 1])
        files.append((f1, f2))
    ref = api.Reference(fa, lib_path=lib_path)
    try:
        out = os.path.join(d, "out")
        st = e2e.run(ref, files, out, pairs_per_batch=max(50, rs.n_pairs // (3 * workers)), bam_threads=2, rec_threads=3, lib_path=lib_path,
                     layout="reference", chunk=chunk, read_groups="S1:L1:1:FC:1,bad")
        names, offs, clens, alt, l_pac = ref.contigs()
        table = api.bucket_table(names, clens, chunk, lib_path=lib_path)
        assert st["files"] == ["bc_sorted_bam.bam"] + table.files
        assert sorted(os.listdir(out)) == sorted(st["files"])
        # the same reads as one batch: the records every file must follow from
        flags = [api.worth_running_rfa(rs.barcodes[b], int(po[b + 1] - po[b])) for b in range(len(po) - 1)]
        b = ref.batch(rs.seqs, rs.lens).run()
        fo = b.fetch()
        c = b.rfa(po, flags)
        pp = b.post()
        tags = b.tags()
        b.free()
    finally:
        ref.close()
    exp = _expected(rs, names, table, c["cands"], c["cand_off"], fo["alns"], fo["cigars"], pp["post"], pp["split"], pp["mm_ref"], pp["mm_read"], tags)
    n_split = int((pp["split"]["split"] >= 0).sum())
    assert n_split >= 2 and st["records"] == 2 * rs.n_pairs + n_split and len(exp) == st["records"]
    got = {f: _read_bam(os.path.join(out, f)) for f in st["files"]}
    text = got["bc_sorted_bam.bam"][0]
    assert "@RG\tID:S1:L1:1:FC:1\tPL:ILLUMINA\tPU:S1:L1:1:FC:1\tLB:L1.1\tSM:S1\tDT:" in text and "ID:bad" not in text
    bc = got["bc_sorted_bam.bam"][1]
    assert len(bc) == len(exp)
    # every record equals the restatement, and it sits in bc_sorted_bam.bam and byte-identical exactly once in its bucket
    where = {}
    for f in table.files:
        for rec in got[f][1]:
            where.setdefault(rec["raw"], []).append(f)
    by_name = {}
    for rec in bc:
        by_name.setdefault(rec["name"], []).append(rec)
    exp_by_name = {}
    for bk, e in exp:
        exp_by_name.setdefault(e["name"], []).append((bk, e))
    assert sorted(by_name) == sorted(exp_by_name)
    n_unmapped = n_sec = 0
    for name, recs in by_name.items():
        assert len(recs) == len(exp_by_name[name])
        for rec, (bk, e) in zip(recs, exp_by_name[name]):
            for key in e:
                assert rec[key] == e[key], (name, key, rec[key], e[key])
            assert where.get(rec["raw"]) == [table.files[bk]], (name, where.get(rec["raw"]), table.files[bk])
            n_unmapped += (rec["flag"] >> 2) & 1
            n_sec += (rec["flag"] >> 8) & 1
    assert n_unmapped >= 1 and n_sec == n_split
    assert sum(len(got[f][1]) for f in table.files) == len(bc)
    # a split record follows its primary, in bc_sorted_bam.bam and in its bucket when both share it
    for i, rec in enumerate(bc):
        if rec["flag"] & 0x100:
            assert i > 0 and bc[i - 1]["name"] == rec["name"] and not bc[i - 1]["flag"] & 0x100 and (bc[i - 1]["flag"] & 0xc0) == (rec["flag"] & 0xc0)
    return rs, exp, got, table, workers


def test_reference_layout_hostsim(sim):
    """One worker: the order inside every file is the write order of DoDumpToBam (reads in batch order, primary then split)."""
    rs, exp, got, table, _ = _layout(sim, 5, 60, 1)
    assert [r["raw"] for r in got["bc_sorted_bam.bam"][1]] == [r["raw"] for r in got["bc_sorted_bam.bam"][1]]
    assert [(r["name"], r["flag"]) for r in got["bc_sorted_bam.bam"][1]] == [(e["name"], e["flag"]) for _, e in exp]
    for k, f in enumerate(table.files):
        assert [(r["name"], r["flag"]) for r in got[f][1]] == [(e["name"], e["flag"]) for bk, e in exp if bk == k], f


def test_default_layout_is_unchanged_by_the_new_argument(sim):
    with pytest.raises(ValueError):
        e2e.run(None, [], "/nonexistent", layout="nope")


@pytest.mark.gpu
def test_reference_layout_gpu(built):
    _layout(api.LIB_PATH, 24, 300, 3)

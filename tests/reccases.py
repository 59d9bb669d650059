"""Shared by tests/test_device_records.py (host double) and tests/test_device_records_gpu.py (product library): a crafted FASTQ workload for
the records phase (arx_batch_records), the HOST path that is the reference of every comparison (arx_recbuf_build -> arx_bam_write on a host
writer, the file inflated block by block as tests/test_bam_sink.py does), and the walks over the inflated stream."""
import ctypes as C
import os
import struct
import zlib

import numpy as np

from arachne_amd import api, synth

ACGT = np.frombuffer(b"ACGTN", dtype=np.uint8)


def inflate(path):
    """the BGZF file block by block -> the uncompressed stream (EOF block included: it inflates to nothing)"""
    raw = open(path, "rb").read()
    out, o = [], 0
    while o < len(raw):
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        out.append(zlib.decompress(raw[o + 18:o + bsize - 8], -15))
        o += bsize
    return b"".join(out)


def header_len(data):
    """bytes of the BAM header (magic, text, references) in front of the first record"""
    l_text = struct.unpack_from("<i", data, 4)[0]
    o = 8 + l_text
    n_ref = struct.unpack_from("<i", data, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 4 + struct.unpack_from("<i", data, o)[0] + 4
    return o


def walk(stream):
    """record start offsets (n + 1) from the block_size fields, and the records' fields"""
    off, recs, o = [0], [], 0
    while o < len(stream):
        bs = struct.unpack_from("<i", stream, o)[0]
        rid, pos, l_name, mapq, bn, n_cig, flag, l_seq, mrid, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", stream, o + 4)
        q = o + 36 + l_name
        cig = np.frombuffer(stream, dtype="<u4", count=n_cig, offset=q)
        q += 4 * n_cig + (l_seq + 1) // 2 + l_seq
        recs.append(dict(pos=pos, flag=flag, l_seq=l_seq, l_name=l_name, ops=set((cig & 15).tolist()), aux=bytes(stream[q:o + 4 + bs])))
        o += 4 + bs
        off.append(o)
    assert o == len(stream)
    return np.array(off, dtype=np.int64), recs


def _rc(a):
    r = a[::-1].copy()
    m = r < 4
    r[m] = 3 - r[m]
    return r


def crafted_pairs(genome, seed=7):
    """-> list of (barcode, header token, rg or None, r1, r2) in barcode order.  The header of a pair with rg is '@<name>/1 BX:Z:<bc> VX:i:1 <rg>';
    one without is the single token '@<name>BX:Z:<bc>' (no second field: the reader leaves the read group empty; the name it keeps is the token
    less its last two bytes)."""
    rng = np.random.default_rng(seed)
    G = genome.seqs[0]
    lens = [18, 19, 25, 33, 50, 64, 75, 99, 100, 101, 127, 128, 149, 150, 151, 200, 201, 249, 250, 254, 255]
    out = []
    k = [0]

    def name(n):
        k[0] += 1
        return ("%dq" % k[0] + "n" * n)[:n]

    def fr(l1, l2, at=None, ins=None):
        ins = int(rng.integers(300, 420)) if ins is None else ins
        ins = max(ins, l1, l2)
        at = int(rng.integers(1000, len(G) - 2000)) if at is None else at
        return G[at:at + l1].copy(), _rc(G[at + ins - l2:at + ins])

    # a barcode with '-': read lengths 18..255 odd and even, names of 1..40 bytes (every residue mod 16), half of the headers without a read group
    for i in range(24):
        l1, l2 = lens[i % len(lens)], lens[(i * 5 + 3) % len(lens)]
        r1, r2 = fr(l1, l2)
        out.append(("AAAC-1", name(1 + i * 17 % 40), None if i & 1 else "S:L:1:FC:%d" % (i % 3), r1, r2))
    # one without '-'
    for i in range(20):
        r1, r2 = fr(lens[(i + 7) % len(lens)], 150)
        out.append(("AAAG", name(3 + i), "rgB", r1, r2))
    # one with '-' that the caller marks not unique (a continuation set): no BX either
    for i in range(20):
        r1, r2 = fr(150, lens[(i + 2) % len(lens)])
        out.append(("AAAT-1", name(5 + i % 16), "rgC", r1, r2))
    # the special cases, in a barcode with '-'
    sp = []
    sp.append((name(254), "rgD", rng.integers(0, 4, 150).astype(np.uint8), rng.integers(0, 4, 151).astype(np.uint8)))    # unmappable: placeholders
    at = 50000
    sp.append((name(9), "rgD", G[at:at + 30].copy(), rng.integers(0, 4, 150).astype(np.uint8)))                          # mapped, unmapped by the score rule
    r1, r2 = fr(130, 150, at=60000)
    sp.append((name(10), "rgD", np.concatenate([rng.integers(0, 4, 20).astype(np.uint8), r1]), r2))                      # soft clip
    at = 70000
    sp.append((name(11), "rgD", np.concatenate([G[at:at + 70], _rc(G[at + 5000:at + 5006]), G[at + 70:at + 145]]), _rc(G[at + 200:at + 350])))   # insertion
    at = 80000
    sp.append((name(12), "rgD", np.concatenate([G[at:at + 70], G[at + 78:at + 158]]), _rc(G[at + 200:at + 350])))        # deletion
    r1, r2 = fr(150, 150, at=90000, ins=350)
    sp.append((name(13), "rgD", r1, r2))
    sp.append((name(14), "rgD", r1.copy(), r2.copy()))                                                                  # an exact duplicate pair
    r1, r2 = fr(101, 150)
    r1[40] = 4                                                                                                          # an N
    sp.append((name(1), "rgD", r1, r2))
    for i in range(8):
        r1, r2 = fr(lens[(3 * i + 1) % len(lens)], lens[(7 * i) % len(lens)])
        sp.append((name(15 + i), "rgD", r1, r2))
    sp.append((name(2), "rgD", fr(150, 150)[0], np.zeros(0, np.uint8)))                                                  # a zero-length read
    out += [("AACA-1",) + x for x in sp]
    return out


def write_fastq(pairs, p1, p2):
    with open(p1, "wb") as f1, open(p2, "wb") as f2:
        for i, (bc, nm, rg, r1, r2) in enumerate(pairs):
            for f, r, mate in ((f1, r1, 1), (f2, r2, 2)):
                hdr = f"@{nm}/{mate} BX:Z:{bc} VX:i:1 {rg}" if rg is not None else f"@{nm}BX:Z:{bc}"
                q = bytes(33 + (j * 7 + i + mate) % 41 for j in range(len(r)))
                f.write(hdr.encode() + b"\n" + ACGT[r].tobytes() + b"\n+\n" + q + b"\n")


def make_index(d, genome, lib_path):
    fa = os.path.join(d, "g.fa")
    genome.write_fasta(fa)
    api.index_build(fa, fa, lib_path=lib_path)
    return fa


def with_unique(sb, v, clear_sets):
    """a copy of the _SuperBatch whose `unique` is cleared for the sets whose barcode is in clear_sets -> (sb2, keep-alive)"""
    n = int(v["n_sets"])
    uniq = np.frombuffer((C.c_uint8 * n).from_address(sb.unique), dtype=np.uint8).copy()
    bo = np.frombuffer((C.c_int64 * (n + 1)).from_address(sb.barcode_off), dtype=np.int64)
    bcs = C.string_at(sb.barcodes, int(bo[-1]))
    for s in range(n):
        if bcs[bo[s]:bo[s + 1]].decode() in clear_sets:
            uniq[s] = 0
    sb2 = api._SuperBatch()
    C.memmove(C.byref(sb2), C.byref(sb), C.sizeof(sb))
    sb2.unique = uniq.ctypes.data
    return sb2, uniq


class Case:
    """One super-batch taken through the path on `ref`, kept at the point where both record paths start: run, rfa and post done, the slabs home."""

    def __init__(self, ref, sb, v, lib_path, penalty=-4):
        self.ref, self.sb, self.v, self.lib_path = ref, sb, v, lib_path
        self.batch = ref.batch(v["bases"], v["lens"]).run()
        self.batch.rfa(v["set_pair_off"], v["do_rfa"], penalty=penalty, fetch=False)
        self.buf = {}
        self.batch.fetch_into(self.buf)
        self.post = self.batch.post_into(self.buf).copy()
        self.rb = api.RecBuf(lib_path=lib_path)

    def host_view(self, dup):
        b = self.buf
        return self.rb.build(self.sb, b["cand_off"], b["cands"], b["alns"], b["cigars"], self.post if dup else None, threads=2)

    def active_pos(self):
        """candidate pos of every read's active candidate (the LAST active one, as RecBuf takes it)"""
        co, ca = self.buf["cand_off"], self.buf["cands"]
        return [int(ca["pos"][[i for i in range(co[r], co[r + 1]) if ca["active"][i]][-1]]) for r in range(2 * int(self.v["n_pairs"]))]

    def free(self):
        self.batch.free()
        self.rb.free()


def host_file(path, ref, lib_path, views):
    """the host path's file: every view through arx_bam_write on a host writer -> the inflated stream"""
    names, offs, clens, alt, l_pac = ref.contigs()
    w = api.BamWriter(path, names, clens, extra_header="@PG\tID:t\n", threads=2, level=1, lib_path=lib_path)
    for view in views:
        w.write_view(view)
    w.close()
    return inflate(path)


def open_writer(path, ref, lib_path, device=None):
    names, offs, clens, alt, l_pac = ref.contigs()
    return api.BamWriter(path, names, clens, extra_header="@PG\tID:t\n", threads=2, level=1, lib_path=lib_path, device=device)

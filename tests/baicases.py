"""Shared by tests/test_bam_index_sim.py (the host program over arachne_amd/csrc/dev_bamindex.h) and tests/test_bam_index_gpu.py (the product's
kernels through arx_selftest_bam_index and arx_bam_index): coordinate-sorted BAM record streams with a block table, each with the .bai the
contract of include/arachne_amd.h (arx_bam_index) asks for.  Nothing here comes from the code under test:
  bai_of(records, hdr, ref_len, blk_at, blk_isize) -> bytes     a serial restatement of the contract, written from its text and from the SAM
                                                                specification's 5.2 and 5.3; raises Refused(code, record, rule)
  read_bai(bytes) / query(bai, raw, rid, beg, end)              an independent reader: the specification's reg2bins and the linear index's
                                                                minimum; over a real file it seeks by virtual offset and returns the records
                                                                of the listed chunks that overlap
  cases() -> {name: Case}; broken() -> {name: Case} (chains that must be refused); check_cases() asserts from the bytes that every case is what
  its name claims."""
import bisect
import functools
import struct
import zlib

import bgzfio
from sortcases import rec

ARX_E_ARG, ARX_E_IO = -2, -5
SEGS = (64, 256, 4096)
OPS = "MIDNSHP=X"
R_FIELDS, R_REFID, R_POS, R_END, R_ORDER = 1, 2, 3, 4, 5          # the rules, as arx_selftest_bam_index numbers them in stats[9]
PSEUDO = 37450


class Refused(Exception):
    def __init__(self, code, record, rule):
        Exception.__init__(self, "code %d record %r rule %r" % (code, record, rule))
        self.code, self.record, self.rule = code, record, rule


def cigar(text):
    """'10M2I' -> the words of a BAM CIGAR"""
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append(int(n) << 4 | OPS.index(ch))
            n = ""
    return tuple(out)


def m(rid, pos, name, cig="10M", **kw):
    return rec(rid, pos, name, cigar=cigar(cig), **kw)


# ---- the SAM specification, 5.3
def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for first, shift in ((1, 26), (9, 23), (73, 20), (585, 17), (4681, 14)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def fields(r):
    """-> (block_size, refID, pos, l_name, n_cigar_op, flag)"""
    bs, rid, pos, l_name, _mq, _bin, n_cig, flag = struct.unpack_from("<iiiBBHHH", r, 0)
    return bs, rid, pos, l_name, n_cig, flag


def interval(r):
    """a record's [beg, end) as the contract states it"""
    bs, rid, pos, l_name, n_cig, flag = fields(r)
    span = 0
    if not flag & 4:
        for w in struct.unpack_from("<%dI" % n_cig, r, 36 + l_name):
            if w & 15 in (0, 2, 3, 7, 8):
                span += w >> 4
    return pos, pos + (span if span > 0 else 1)


def voffsets(blk_at, blk_isize):
    """-> (V, total): V(o) for an inflated offset o <= total"""
    ooff, o = [], 0
    for s in blk_isize:
        ooff.append(o)
        o += s
    total = o
    full = [b for b, s in enumerate(blk_isize) if s > 0]
    starts = [ooff[b] for b in full]

    def V(o):
        assert 0 <= o <= total
        if o == total:
            return blk_at[full[-1] + 1 if full else len(blk_isize)] << 16
        b = full[bisect.bisect_right(starts, o) - 1]
        assert ooff[b] <= o < ooff[b] + blk_isize[b]
        return blk_at[b] << 16 | (o - ooff[b])
    return V, total


def bai_of(records, hdr, ref_len, blk_at, blk_isize):
    n_ref = len(ref_len)
    for i, l in enumerate(ref_len):
        if l > 1 << 29:
            raise Refused(ARX_E_ARG, None, "contig %d is longer than 2^29" % i)
    if any(a >= 1 << 48 for a in blk_at):
        raise Refused(ARX_E_ARG, None, "a file offset of 2^48 or more")
    V, total = voffsets(blk_at, blk_isize)
    bins = [dict() for _ in range(n_ref)]
    lin = [dict() for _ in range(n_ref)]
    span = [None] * n_ref                     # [V(first record), end of the last]
    counts = [[0, 0] for _ in range(n_ref)]
    n_no_coor, o, prev, run = 0, hdr, None, None
    for k, r in enumerate(records):
        bs, rid, pos, l_name, n_cig, flag = fields(r)
        bad = []
        if 36 + l_name + 4 * n_cig > 4 + bs:
            raise Refused(ARX_E_IO, k, R_FIELDS)
        key = (rid & 0xFFFFFFFF, pos)
        if prev is not None and key < prev:
            bad.append(R_ORDER)
        prev = key
        if not -1 <= rid < n_ref:
            bad.append(R_REFID)
        elif rid >= 0:
            if pos < 0:
                bad.append(R_POS)
            elif interval(r)[1] > ref_len[rid]:
                bad.append(R_END)
        if bad:
            raise Refused(ARX_E_ARG, k, min(bad))
        vb, ve = V(o), V(o + len(r))
        o += len(r)
        if rid < 0:
            n_no_coor += 1
            run = None
            continue
        beg, end = interval(r)
        b = reg2bin(beg, end)
        chunks = bins[rid].setdefault(b, [])
        if run == (rid, b):
            chunks[-1][1] = ve                                   # the run goes on
        elif chunks and chunks[-1][1] >> 16 >= vb >> 16:
            chunks[-1][1] = ve                                   # a new run, joined to the bin's last chunk
        else:
            chunks.append([vb, ve])
        run = (rid, b)
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            lin[rid][w] = min(lin[rid].get(w, vb), vb)
        counts[rid][1 if flag & 4 else 0] += 1
        span[rid] = [vb if span[rid] is None else span[rid][0], ve]
    assert o == total, (o, total)
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for i in range(n_ref):
        out.append(struct.pack("<i", len(bins[i]) + (1 if span[i] else 0)))
        for b in sorted(bins[i]):
            out.append(struct.pack("<Ii", b, len(bins[i][b])))
            out.extend(struct.pack("<QQ", c[0], c[1]) for c in bins[i][b])
        if span[i]:
            out.append(struct.pack("<IiQQQQ", PSEUDO, 2, span[i][0], span[i][1], counts[i][0], counts[i][1]))
        n_intv = 1 + max(lin[i]) if lin[i] else 0
        out.append(struct.pack("<i", n_intv))
        vals, nxt = [0] * n_intv, None
        for w in range(n_intv - 1, -1, -1):
            nxt = lin[i].get(w, nxt)
            vals[w] = nxt
        out.extend(struct.pack("<Q", v) for v in vals)
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


# ---- the independent reader and query
def read_bai(data):
    assert data[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", data, 4)
    o, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", data, o)
        o += 4
        bins, pseudo, order = {}, None, []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, o)
            o += 8
            chunks = [struct.unpack_from("<QQ", data, o + 16 * c) for c in range(n_chunk)]
            o += 16 * n_chunk
            order.append(b)
            if b == PSEUDO:
                assert n_chunk == 2
                pseudo = chunks
            else:
                assert b < PSEUDO and n_chunk >= 1 and b not in bins
                assert all(c[0] < c[1] for c in chunks) and all(x[1] <= y[0] for x, y in zip(chunks, chunks[1:]))
                bins[b] = chunks
        assert order == sorted(order)                                          # ascending, the pseudo-bin last
        n_intv, = struct.unpack_from("<i", data, o)
        o += 4
        lin = list(struct.unpack_from("<%dQ" % n_intv, data, o))
        o += 8 * n_intv
        assert lin == sorted(lin)
        refs.append(dict(bins=bins, pseudo=pseudo, lin=lin))
    n_no_coor, = struct.unpack_from("<Q", data, o)
    assert o + 8 == len(data)
    return dict(refs=refs, n_no_coor=n_no_coor)


class VReader:
    """the records of a BGZF file from a virtual offset on"""
    def __init__(self, raw):
        self.blocks = bgzfio.split(raw)
        self.at = [b["at"] for b in self.blocks]
        self.size = len(raw)
        self.cache = {}

    def data(self, i):
        if i not in self.cache:
            self.cache[i] = zlib.decompress(self.blocks[i]["payload"], -15)
        return self.cache[i]

    def seek(self, v):
        self.i, self.u = self.at.index(v >> 16), v & 0xffff

    def tell(self):
        while self.i < len(self.blocks) and self.u >= len(self.data(self.i)):  # behind a block's last byte is the next non-empty block's first
            self.i, self.u = self.i + 1, 0
        return (self.at[self.i] if self.i < len(self.blocks) else self.size) << 16 | self.u

    def read(self, n):
        out = b""
        while len(out) < n:
            self.tell()
            assert self.i < len(self.blocks), "the file ends inside a record"
            piece = self.data(self.i)[self.u:self.u + n - len(out)]
            self.u += len(piece)
            out += piece
        return out

    def record(self):
        head = self.read(4)
        return head + self.read(struct.unpack("<i", head)[0])


def query(bai, raw, rid, beg, end):
    """the records of contig rid that overlap [beg, end), found the way a reader of the index finds them"""
    ref = bai["refs"][rid]
    w = beg >> 14
    if w >= len(ref["lin"]):
        return []                                # no record reaches that window
    min_off = ref["lin"][w]
    chunks = []
    for cb, ce in sorted(c for b in reg2bins(beg, end) for c in ref["bins"].get(b, []) if c[1] > min_off):
        cb = max(cb, min_off)
        if chunks and cb <= chunks[-1][1]:       # a joined chunk spans the records of other bins between its runs: file ranges that overlap are read once
            chunks[-1][1] = max(chunks[-1][1], ce)
        else:
            chunks.append([cb, ce])
    rd, out = VReader(raw), []
    for cb, ce in chunks:
        rd.seek(cb)
        while rd.tell() < ce:
            r = rd.record()
            _bs, rrid, pos, _ln, _nc, _fl = fields(r)
            rb, re_ = interval(r)
            if rrid == rid and rb < end and re_ > beg:
                out.append(r)
    return out


def brute(records, rid, beg, end):
    return [r for r in records if fields(r)[1] == rid and interval(r)[0] < end and interval(r)[1] > beg]


# ---- the cases
class Case:
    """records behind hdr bytes of header, a block table (isize per block; at: synthetic file offsets from at0 on), the slab sizes to run at"""
    def __init__(self, recs, ref_len, isize=113, hdr=0, at0=0, eof=1, slabs=(113, 400, 2000)):
        self.recs, self.ref_len, self.hdr, self.slabs = list(recs), list(ref_len), hdr, tuple(slabs) + (0,)
        self.stream = bytes(0xEE for _ in range(hdr)) + b"".join(self.recs)
        n = len(self.stream)
        if isinstance(isize, int):
            isize = [min(isize, n - o) for o in range(0, n, isize)]
        self.isize = list(isize) + [0] * eof
        assert sum(self.isize) == n and all(0 <= s <= 65536 for s in self.isize)
        self.at = [at0]
        for b, s in enumerate(self.isize):
            self.at.append(self.at[-1] + 26 + s // 2 + b % 3)
        self.off = [hdr]
        for r in self.recs:
            self.off.append(self.off[-1] + len(r))
        try:
            self.want, self.refused = bai_of(self.recs, hdr, self.ref_len, self.at, self.isize), None
        except Refused as e:
            self.want, self.refused = None, e

    def cuts(self):
        out, o = [], 0
        for s in self.isize:
            o += s
            out.append(o)
        return out

    def packed(self):
        """the case file of tests/baisim/bam_index_sim.cpp"""
        words = [len(self.stream), self.hdr, len(self.ref_len), len(self.isize)] + self.ref_len + self.at + self.isize
        return struct.pack("<%dq" % len(words), *words) + self.stream


def sizes_to(*cuts_and_end):
    """block sizes from ascending cut offsets, the last being the stream's length"""
    return [b - a for a, b in zip((0,) + cuts_and_end[:-1], cuts_and_end)]


BIG = 1 << 29
LEAF = [m(0, 20000, b"l0"), m(0, 20010, b"l1"), m(0, 20020, b"parent", "20000M"), m(0, 20030, b"l2"), m(0, 20040, b"l3")]


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["empty"] = Case([], [1000, 2000], isize=[], eof=0)
    c["header_only"] = Case([], [1000], hdr=40)
    c["one_record"] = Case([m(0, 7, b"q")], [1000])
    c["only_unplaced"] = Case([rec(-1, -1, b"u%d" % k, l_seq=k) for k in range(5)], [1000, 2000])
    c["pos_zero"] = Case([m(0, 0, b"z"), m(0, 0, b"z2", "5M")], [1000])
    c["ends_16384_16385"] = Case([m(0, 16374, b"a"), m(0, 16375, b"b")], [40000])
    edge = []
    for sh in (14, 17, 20, 23, 26):
        edge += [m(0, (1 << sh) - 10, b"on%d" % sh), m(0, (1 << sh) - 5, b"x%d" % sh), m(0, 1 << sh, b"at%d" % sh)]
    c["level_borders"] = Case(edge, [BIG], hdr=57)
    c["contig_2_29"] = Case([m(0, 5, b"a"), m(0, BIG - 50, b"end", "50M")], [BIG])
    c["every_op"] = Case([m(0, 100, b"ops", "5M3I4D100N6S2H1P7=8X", l_seq=29), m(0, 300, b"clip", "10I5S", l_seq=15), m(1, 0, b"n", "10M1000000N10M", l_seq=20),
                          m(1, 500, b"i", "3S4M")], [5000, 2000000])
    c["placed_unmapped"] = Case([m(0, 10, b"map"), rec(0, 10, b"un", flag=4 | 1 | 8), m(0, 20, b"unc", "50M", flag=4), rec(1, 16383, b"un2", flag=4),
                                 m(1, 16383, b"mate2", "2M"), rec(-1, -1, b"un3", flag=4)], [60, 16385])
    c["empty_contigs"] = Case([m(1, 5, b"a"), m(1, 9, b"b"), m(3, 0, b"c")], [100, 200, 300, 400, 500])
    c["unset_windows"] = Case([m(0, 100000, b"a"), m(0, 100005, b"b"), m(0, 300000, b"c"), m(1, 16384 * 3, b"d")], [400000, 100000])
    n = sum(len(r) for r in LEAF)
    c["leaf_resumed_one_block"] = Case(LEAF, [100000], isize=[n])
    c["leaf_resumed_two_blocks"] = Case(LEAF, [100000], isize=sizes_to(len(LEAF[0]) + len(LEAF[1]) + len(LEAF[2]), n))
    for k in (255, 256, 257):
        c["records_%d" % k] = Case([m(0, 7 + j // 3, b"r%d" % j) for j in range(k)], [1000], slabs=(2000, 5000, 9000))
        c["runs_%d" % k] = Case([m(0, 16384 * j, b"r%d" % j) for j in range(k)], [16384 * 300], slabs=(2000, 5000, 9000))
    body = [m(0, 10 + k, b"b%d" % k, l_seq=k % 5) for k in range(12)]
    off = [0]
    for r in body:
        off.append(off[-1] + len(r))
    n = off[-1]
    c["start_on_first_byte"] = Case(body, [1000], isize=sizes_to(off[4], off[7], n), slabs=(1, 200, 300))
    c["start_on_last_byte"] = Case(body, [1000], isize=sizes_to(off[4] + 1, off[7] + 1, n), slabs=(1, 200, 300))
    c["block_size_cut"] = Case(body, [1000], isize=sizes_to(off[3] + 1, off[5] + 2, off[8] + 3, n), slabs=(1, 150, 250))
    c["empty_blocks_behind"] = Case(body, [1000], isize=sizes_to(off[4], off[4], off[9], off[9], off[9], n), slabs=(1, 200, 300), eof=2)
    c["one_byte_blocks"] = Case(body[:3], [1000], isize=1, slabs=(3, 7, 50))
    c["no_eof_block"] = Case(body, [1000], eof=0)
    c["at_above_2_32"] = Case(body, [1000], at0=(1 << 32) + 12345)
    c["at_near_2_48"] = Case(body, [1000], at0=(1 << 48) - 2000)
    r = m(0, 50, b"somename", "3M2I4M1D5M", l_seq=14)
    pre = [m(0, 40, b"p")]
    p = len(pre[0])
    for name, cut in (("slab_cuts_fixed", p + 20), ("slab_cuts_name", p + 36 + 4), ("slab_cuts_cigar", p + 36 + 9 + 6), ("slab_cuts_between", p)):
        tail = [m(0, 60, b"t")]
        c[name] = Case(pre + [r] + tail, [1000], isize=sizes_to(cut, p + len(r) + len(tail[0])), slabs=(1, 1, 1))
    long_cig = "".join("%dM%dI" % (1 + k % 3, 1 + k % 2) for k in range(200))
    c["longer_than_a_slab"] = Case([m(0, 3, b"a"), m(0, 4, b"long", long_cig, l_seq=900), m(0, 4, b"b"), m(1, 0, b"c")], [5000, 100], slabs=(113, 400, 1000))
    # refusals of single records
    good = [m(0, 10 + k, b"g%d" % k) for k in range(8)]
    g = [0]
    for x in good:
        g.append(g[-1] + len(x))
    c["refuse_order"] = Case(good[:5] + [m(0, 3, b"early")] + good[5:], [1000])
    c["refuse_order_at_slab_border"] = Case(good[:4] + [m(0, 3, b"early")] + good[4:], [1000], isize=sizes_to(g[4], g[-1] + len(m(0, 3, b"early"))), slabs=(1, g[4], g[4] + 1))
    c["refuse_order_unplaced_first"] = Case([rec(-1, -1, b"u")] + good, [1000])
    c["refuse_refid_n_ref"] = Case(good + [m(1, 0, b"r")], [1000])
    c["refuse_refid_minus_2"] = Case(good + [m(-2, 0, b"r")], [1000])
    c["refuse_negative_pos"] = Case([m(0, -1, b"n")] + good, [1000])
    c["refuse_end_beyond_contig"] = Case(good + [m(0, 995, b"e", "6M")], [1000])
    c["refuse_long_contig"] = Case(good, [1000, BIG + 1])
    return c


@functools.lru_cache(maxsize=None)
def broken():
    """chains that break: the stream is not a list of records, so the expected code is stated here -- ARX_E_IO"""
    good = [m(0, 10 + k, b"g%d" % k) for k in range(8)]
    s = b"".join(good)
    at = sum(len(r) for r in good[:5])
    out = {}
    for name, t in (("block_size_10", s[:at] + struct.pack("<i", 10) + s[at + 4:]), ("last_record_past_the_end", s[:-5])):
        c = Case([], [1000], isize=[], eof=0)
        c.stream = t
        c.isize = [min(113, len(t) - o) for o in range(0, len(t), 113)] + [0]
        c.at = [0]
        for b, z in enumerate(c.isize):
            c.at.append(c.at[-1] + 30 + z)
        out[name] = c
    bad = bytearray(m(0, 30, b"nofit", "4M"))
    bad[12] = 200                                                        # a name that block_size does not hold
    out["name_past_block_size"] = Case(good + [bytes(bad)], [1000])
    return out


def check_cases():
    c = cases()
    for name, k in c.items():
        keys = [(fields(r)[1] & 0xFFFFFFFF, fields(r)[2]) for r in k.recs]
        assert (keys == sorted(keys)) == (not name.startswith("refuse_order")), name
        assert (k.refused is not None) == name.startswith("refuse_"), name
        if k.refused is None:
            bai = read_bai(k.want)
            assert len(bai["refs"]) == len(k.ref_len)
            placed = sum(sum(r["pseudo"][1]) for r in bai["refs"] if r["pseudo"])
            assert placed + bai["n_no_coor"] == len(k.recs), name
        assert len(k.slabs) == 4 and k.slabs[-1] == 0
    assert c["empty"].stream == b"" and c["empty"].isize == [] and read_bai(c["empty"].want)["refs"] == [dict(bins={}, pseudo=None, lin=[])] * 2
    assert len(c["one_record"].recs) == 1 and read_bai(c["only_unplaced"].want)["n_no_coor"] == 5
    assert [interval(r) for r in c["pos_zero"].recs] == [(0, 10), (0, 5)]
    assert [interval(r)[1] for r in c["ends_16384_16385"].recs] == [16384, 16385]
    assert [reg2bin(*interval(r)) for r in c["ends_16384_16385"].recs] == [4681, 585]
    lb = {fields(r)[2]: reg2bin(*interval(r)) for r in c["level_borders"].recs}
    for sh, parent in ((14, 585), (17, 73), (20, 9), (23, 1), (26, 0)):
        assert lb[(1 << sh) - 10] == 4681 + (((1 << sh) - 10) >> 14) and lb[1 << sh] == 4681 + (1 << sh >> 14)        # up to the border, and from it
        assert lb[(1 << sh) - 5] == parent                                                                           # across it: the first bin a level up
    assert lb[(1 << 26) - 5] == 0
    assert c["contig_2_29"].ref_len == [1 << 29] and interval(c["contig_2_29"].recs[-1])[1] == 1 << 29
    ops = c["every_op"].recs
    assert {w & 15 for w in cigar("5M3I4D100N6S2H1P7=8X")} == set(range(9)) and interval(ops[0]) == (100, 100 + 5 + 4 + 100 + 7 + 8)
    assert interval(ops[1]) == (300, 301) and interval(ops[2]) == (0, 1000020)
    assert len(read_bai(c["every_op"].want)["refs"][1]["lin"]) == 62 and reg2bin(0, 1000020) == 73
    pu = c["placed_unmapped"]
    assert [interval(r) for r in pu.recs[1:4]] == [(10, 11), (20, 21), (16383, 16384)] and fields(pu.recs[2])[4] == 1
    assert [r["pseudo"][1] for r in read_bai(pu.want)["refs"]] == [(1, 2), (1, 1)] and read_bai(pu.want)["n_no_coor"] == 1
    ec = read_bai(c["empty_contigs"].want)["refs"]
    assert [bool(r["bins"]) for r in ec] == [False, True, False, True, False] and [len(r["lin"]) for r in ec] == [0, 1, 0, 1, 0]
    uw = read_bai(c["unset_windows"].want)["refs"]
    assert len(uw[0]["lin"]) == 19 and uw[0]["lin"][0] == uw[0]["lin"][6] < uw[0]["lin"][7] == uw[0]["lin"][18] and len(uw[1]["lin"]) == 4
    one, two = read_bai(c["leaf_resumed_one_block"].want)["refs"][0]["bins"], read_bai(c["leaf_resumed_two_blocks"].want)["refs"][0]["bins"]
    assert sorted(one) == sorted(two) == [585, 4682] and len(one[4682]) == 1 and len(two[4682]) == 2          # joined in one block, apart in two
    for n in (255, 256, 257):
        assert len(c["records_%d" % n].recs) == n and len(read_bai(c["runs_%d" % n].want)["refs"][0]["bins"]) == n
    assert all(x in c["start_on_first_byte"].off for x in c["start_on_first_byte"].cuts()[:2])
    assert all(x - 1 in c["start_on_last_byte"].off for x in c["start_on_last_byte"].cuts()[:2])
    bc = c["block_size_cut"]
    assert [min(x - o for o in bc.off if o <= x) for x in bc.cuts()[:3]] == [1, 2, 3]
    eb = c["empty_blocks_behind"]
    assert eb.isize.count(0) == 5 and eb.isize[1] == 0 and eb.isize[3] == eb.isize[4] == 0 and eb.cuts()[0] in eb.off and eb.cuts()[2] in eb.off
    assert set(c["one_byte_blocks"].isize) == {0, 1} and c["no_eof_block"].isize[-1] > 0
    assert c["at_above_2_32"].at[0] > 1 << 32 and (1 << 48) - 65536 * 2 < c["at_near_2_48"].at[-1] < 1 << 48 and c["at_near_2_48"].at[-1] >= 1 << 47
    r0 = c["slab_cuts_fixed"].off[1]
    assert c["slab_cuts_fixed"].cuts()[0] - r0 == 20 and c["slab_cuts_name"].cuts()[0] - r0 == 40 and c["slab_cuts_cigar"].cuts()[0] - r0 == 36 + 9 + 6
    assert c["slab_cuts_between"].cuts()[0] == r0 and fields(c["slab_cuts_fixed"].recs[1])[3:5] == (9, 5)
    lg = c["longer_than_a_slab"]
    assert 36 + 5 + 4 * fields(lg.recs[1])[4] > max(lg.slabs) and len(lg.recs[1]) > 2 * max(lg.slabs)
    for name, rule, record in (("refuse_order", R_ORDER, 5), ("refuse_order_at_slab_border", R_ORDER, 4), ("refuse_order_unplaced_first", R_ORDER, 1), ("refuse_refid_n_ref", R_REFID, 8),
                               ("refuse_refid_minus_2", R_REFID, 8), ("refuse_negative_pos", R_POS, 0), ("refuse_end_beyond_contig", R_END, 8)):
        e = c[name].refused
        assert (e.code, e.rule, e.record) == (ARX_E_ARG, rule, record), (name, e)
    sb = c["refuse_order_at_slab_border"]
    assert sb.cuts()[0] == sb.off[4] and sb.slabs[1] == sb.isize[0]                   # the offender is a slab's first record
    assert c["refuse_long_contig"].refused.code == ARX_E_ARG and c["refuse_long_contig"].refused.record is None
    assert interval(c["refuse_end_beyond_contig"].recs[-1])[1] == 1001
    for name, k in broken().items():
        if name == "name_past_block_size":
            assert k.refused.code == ARX_E_IO and k.refused.rule == R_FIELDS

"""Shared by tests/test_bam_index_csi_sim.py (the host program over arachne_amd/csrc/dev_bamindex.h) and tests/test_bam_index_csi_gpu.py (the
product's kernels through arx_selftest_bam_index_csi and arx_bam_index_csi): coordinate-sorted BAM record streams with a block table, each with
the inflated bytes of the .csi that the contract of include/arachne_amd.h (arx_bam_index_csi) asks for.  The record helpers, the block tables
and the refusals are baicases'; nothing here comes from the code under test:
  scheme(min_shift, ref_len) -> (min_shift, depth); reg2bin / reg2bins / meta_bin for any scheme, from the contract's text and CSIv1
  csi_of(records, hdr, ref_len, blk_at, blk_isize, min_shift) -> bytes    a serial restatement of the contract; raises baicases.Refused
  read_csi(bytes) / query(csi, reader, rid, beg, end)                     an independent reader: reg2bins over all levels, the lower bound
                                                                          found by htslib's walk from the leaf bin of beg to the previous
                                                                          sibling or the parent until a bin exists; the records of the listed
                                                                          chunks that overlap, read by virtual offset (StreamReader over a
                                                                          case's table, baicases.VReader over a real file)
  same_as_bai(csi_bytes, bai_bytes)                                       at (14, 5): the BAI's bins and chunks, chunk for chunk, and
                                                                          loffset(4681 + w) = lin[w]
  cases() -> {name: Case}; check_cases() asserts from the bytes that every case is what its name claims and runs the reader over every
  accepted case against baicases.brute."""
import bisect
import functools
import struct

import baicases as bc
from baicases import ARX_E_ARG, ARX_E_IO, R_END, R_FIELDS, R_ORDER, R_POS, R_REFID, Refused, fields, interval, m, rec, sizes_to, voffsets

SEGS = bc.SEGS
TOP = (1 << 31) - 1                                                # the longest contig a BAM header can state
BAI_MAX = 1 << 29


# ---- the scheme (the contract: scheme, bin, meta-bin)
def scheme(min_shift, ref_len):
    if min_shift == 0:
        min_shift = 14
    if not 10 <= min_shift <= 24:
        raise Refused(ARX_E_ARG, None, "min_shift %d" % min_shift)
    depth = 5
    while 1 << (min_shift + 3 * depth) < max(ref_len, default=0):
        depth += 1
    return min_shift, depth


def first_bin(level):
    return (8 ** level - 1) // 7


def meta_bin(depth):
    return first_bin(depth + 1) + 1


def reg2bin(beg, end, min_shift, depth):
    end -= 1
    for level in range(depth, 0, -1):
        s = min_shift + 3 * (depth - level)
        if beg >> s == end >> s:
            return first_bin(level) + (beg >> s)
    return 0


def reg2bins(beg, end, min_shift, depth):
    end -= 1
    out = []
    for level in range(depth + 1):
        s = min_shift + 3 * (depth - level)
        out.extend(range(first_bin(level) + (beg >> s), first_bin(level) + (end >> s) + 1))
    return out


def level_of(b):
    level = 0
    while first_bin(level + 1) <= b:
        level += 1
    return level


def first_window(b, depth):
    level = level_of(b)
    return (b - first_bin(level)) << (3 * (depth - level))


def csi_of(records, hdr, ref_len, blk_at, blk_isize, min_shift):
    n_ref = len(ref_len)
    min_shift, depth = scheme(min_shift, ref_len)
    if any(a >= 1 << 48 for a in blk_at):
        raise Refused(ARX_E_ARG, None, "a file offset of 2^48 or more")
    V, total = voffsets(blk_at, blk_isize)
    bins = [dict() for _ in range(n_ref)]
    win = [dict() for _ in range(n_ref)]
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
        b = reg2bin(beg, end, min_shift, depth)
        chunks = bins[rid].setdefault(b, [])
        if run == (rid, b):
            chunks[-1][1] = ve                                   # the run goes on
        elif chunks and chunks[-1][1] >> 16 >= vb >> 16:
            chunks[-1][1] = ve                                   # a new run, joined to the bin's last chunk
        else:
            chunks.append([vb, ve])
        run = (rid, b)
        for w in range(beg >> min_shift, ((end - 1) >> min_shift) + 1):
            win[rid][w] = min(win[rid].get(w, vb), vb)
        counts[rid][1 if flag & 4 else 0] += 1
        span[rid] = [vb if span[rid] is None else span[rid][0], ve]
    assert o == total, (o, total)
    out = [b"CSI\1", struct.pack("<iiii", min_shift, depth, 0, n_ref)]
    for i in range(n_ref):
        out.append(struct.pack("<i", len(bins[i]) + (1 if span[i] else 0)))
        set_windows = sorted(win[i])
        for b in sorted(bins[i]):
            at = bisect.bisect_left(set_windows, first_window(b, depth))        # the bin's first window, or the next set one above it
            out.append(struct.pack("<IQi", b, win[i][set_windows[at]], len(bins[i][b])))
            out.extend(struct.pack("<QQ", c[0], c[1]) for c in bins[i][b])
        if span[i]:
            out.append(struct.pack("<IQiQQQQ", meta_bin(depth), 0, 2, span[i][0], span[i][1], counts[i][0], counts[i][1]))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


# ---- the independent reader and query
def read_csi(data):
    assert data[:4] == b"CSI\1"
    min_shift, depth, l_aux, n_ref = struct.unpack_from("<iiii", data, 4)
    assert l_aux == 0 and 10 <= min_shift <= 24 and 0 <= depth <= 7
    o, refs = 20, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", data, o)
        o += 4
        bins, loff, meta, order = {}, {}, None, []
        for _ in range(n_bin):
            b, lo, n_chunk = struct.unpack_from("<IQi", data, o)
            o += 16
            chunks = [struct.unpack_from("<QQ", data, o + 16 * c) for c in range(n_chunk)]
            o += 16 * n_chunk
            order.append(b)
            if b == meta_bin(depth):
                assert n_chunk == 2 and lo == 0
                meta = chunks
            else:
                assert b < first_bin(depth + 1) and n_chunk >= 1 and b not in bins
                assert all(c[0] < c[1] for c in chunks) and all(x[1] <= y[0] for x, y in zip(chunks, chunks[1:]))
                assert lo <= chunks[0][0]                                        # no record of the bin starts in front of its loffset
                bins[b], loff[b] = chunks, lo
        assert order == sorted(order) and (meta is not None) == bool(n_bin)      # ascending, the meta-bin last in a contig that holds a record
        refs.append(dict(bins=bins, loff=loff, meta=meta))
    n_no_coor, = struct.unpack_from("<Q", data, o)
    assert o + 8 == len(data)
    return dict(min_shift=min_shift, depth=depth, refs=refs, n_no_coor=n_no_coor)


class StreamReader:
    """the records of a case's stream from a virtual offset of its block table on (baicases.VReader's interface)"""
    def __init__(self, case):
        self.s, self.at = case.stream, case.at
        self.V, self.total = voffsets(case.at, case.isize)
        self.ooff, o = [], 0
        for z in case.isize:
            self.ooff.append(o)
            o += z
        self.o = 0

    def seek(self, v):
        b = self.at.index(v >> 16)
        self.o = (self.ooff[b] if b < len(self.ooff) else self.total) + (v & 0xffff)

    def tell(self):
        return self.V(self.o)

    def record(self):
        bs, = struct.unpack_from("<i", self.s, self.o)
        r = self.s[self.o:self.o + 4 + bs]
        assert len(r) == 4 + bs, "the stream ends inside a record"
        self.o += len(r)
        return r


def lower_bound(csi, rid, beg):
    """htslib's walk: from the leaf bin of beg to the previous sibling, from a first sibling to the parent, until a bin exists -> its loffset,
    or 0 where bin 0 is reached and does not exist"""
    ref, depth = csi["refs"][rid], csi["depth"]
    b = first_bin(depth) + (beg >> csi["min_shift"])
    while b and b not in ref["bins"]:
        parent = (b - 1) >> 3
        b = b - 1 if b > (parent << 3) + 1 else parent
    return ref["loff"].get(b, 0)


def query(csi, reader, rid, beg, end, bounds=None):
    """the records of contig rid that overlap [beg, end), found the way a reader of the index finds them; bounds (a list) collects the lower
    bound that was used"""
    ref = csi["refs"][rid]
    min_off = lower_bound(csi, rid, beg)
    if bounds is not None:
        bounds.append(min_off)
    chunks = []
    for cb, ce in sorted(c for b in reg2bins(beg, end, csi["min_shift"], csi["depth"]) for c in ref["bins"].get(b, []) if c[1] > min_off):
        cb = max(cb, min_off)
        if chunks and cb <= chunks[-1][1]:       # file ranges that overlap are read once
            chunks[-1][1] = max(chunks[-1][1], ce)
        else:
            chunks.append([cb, ce])
    out = []
    for cb, ce in chunks:
        reader.seek(cb)
        while reader.tell() < ce:
            r = reader.record()
            rb, re_ = interval(r)
            if fields(r)[1] == rid and rb < end and re_ > beg:
                out.append(r)
    return out


def same_as_bai(csi_bytes, bai_bytes):
    """a .csi at (14, 5) against the .bai of the same stream: the BAI's bins and chunks, chunk for chunk, the meta-bin its pseudo-bin, and the
    loffset of every leaf bin 4681 + w the linear index's entry w"""
    csi, bai = read_csi(csi_bytes), bc.read_bai(bai_bytes)
    assert (csi["min_shift"], csi["depth"]) == (14, 5) and meta_bin(5) == bc.PSEUDO and csi["n_no_coor"] == bai["n_no_coor"]
    assert len(csi["refs"]) == len(bai["refs"])
    leaves = 0
    for c, b in zip(csi["refs"], bai["refs"]):
        assert c["bins"] == b["bins"] and c["meta"] == b["pseudo"]
        for bn, lo in c["loff"].items():
            if bn >= 4681:
                assert lo == b["lin"][bn - 4681], bn
                leaves += 1
    return leaves


# ---- the cases
class Case(bc.Case):
    """baicases.Case with a min_shift: want is the .csi's inflated bytes; bai the .bai's where the header allows one"""
    def __init__(self, recs, ref_len, min_shift=14, **kw):
        bc.Case.__init__(self, recs, ref_len, **kw)
        self.min_shift, self.bai = min_shift, self.want
        try:
            self.want, self.refused = csi_of(self.recs, self.hdr, self.ref_len, self.at, self.isize, min_shift), None
        except Refused as e:
            self.want, self.refused = None, e


def packed(case, min_shift):
    """the case file of tests/csisim/bam_index_csi_sim.cpp"""
    words = [len(case.stream), case.hdr, len(case.ref_len), len(case.isize), min_shift] + case.ref_len + case.at + case.isize
    return struct.pack("<%dq" % len(words), *words) + case.stream


G30 = 1 << 30
INHERITED_BAI = ("level_borders", "every_op", "leaf_resumed_two_blocks")           # the three the host program also indexes as a .bai


def inherited(k, **kw):
    """a case of baicases with its very block table"""
    return Case(k.recs, k.ref_len, isize=k.isize, eof=0, hdr=k.hdr, at0=k.at[0], slabs=k.slabs[:-1], **kw)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    # 1. baicases' own, at min_shift 14: the BAI's scheme
    for name, k in bc.cases().items():
        if k.refused is None:
            c["bai_" + name] = inherited(k)
    # 2. the depth's edges
    few = lambda top: [m(0, 5, b"a"), m(0, 70000, b"b", "30M5D30M"), m(0, top - 50, b"end", "50M")]
    c["depth5_at_2_29"] = Case(few(BAI_MAX), [BAI_MAX, 1000], hdr=31)
    c["depth6_at_2_29_plus_1"] = Case(few(BAI_MAX + 1), [1000, BAI_MAX + 1][::-1], hdr=31)
    c["depth6_at_2_31_minus_1"] = Case(few(TOP), [TOP], hdr=31)
    c["depth7_at_shift_12"] = Case(few(TOP), [TOP], 12, hdr=31)
    c["depth5_at_shift_16"] = Case(few(TOP), [TOP], 16, hdr=31)
    # 3. the borders of every level at depth 6
    edge = []
    for sh in (14, 17, 20, 23, 26, 29):
        edge += [m(0, (1 << sh) - 10, b"on%d" % sh), m(0, (1 << sh) - 5, b"x%d" % sh), m(0, 1 << sh, b"at%d" % sh)]
    edge.append(m(0, BAI_MAX + 1000, b"spliced", "10M100000000N10M", l_seq=20))
    c["level_borders_depth6"] = Case(edge, [TOP], hdr=57)
    # 4. bins above 65,535: a run key that keeps 16 bits of the bin merges the first pair and confuses the second
    p = 5 * 16384 + 100
    c["bins_65536_apart"] = Case([m(0, 10, b"lead"), m(0, p, b"w"), m(0, p + G30, b"w65536"), m(0, p + G30 + 10, b"w65536b")], [TOP], hdr=20)
    c["bins_65536_apart_two_contigs"] = Case([m(0, 10, b"lead"), m(0, p + G30, b"r0"), m(1, p, b"r1"), m(1, p + 3, b"r1b")], [TOP, TOP], hdr=20)
    # 5. loffset
    k17 = 9 << 17
    c["loffset_backfilled"] = Case([m(0, 100, b"first"), m(0, G30 + k17 + 4 * 16384 - 5, b"mid"), m(0, G30 + k17 + 4 * 16384 + 20, b"leaf")], [TOP], hdr=40)
    c["loffset_parent_first"] = Case([m(0, 7, b"first"), m(0, G30 + 20000, b"parent", "20000M"), m(0, G30 + 20010, b"l0"), m(0, G30 + 20020, b"l1"), m(0, G30 + 50000, b"l2")], [TOP], hdr=40)
    c["loffset_unset_windows"] = Case([m(0, 100000, b"a"), m(0, 100005, b"b"), m(0, 300000, b"c"), m(0, G30 + 300000, b"d"), m(0, G30 + 16384 * 40, b"e"), m(1, 16384 * 3, b"f")],
                                      [TOP, 100000], hdr=40)
    leaf = [m(0, 3, b"first")] + [m(0, G30 + fields(r)[2], b"L%d" % j, "20000M" if j == 2 else "10M") for j, r in enumerate(bc.LEAF)]
    n = sum(len(r) for r in leaf)
    c["leaf_resumed_one_block"] = Case(leaf, [BAI_MAX + 1 + G30], isize=[n])
    c["leaf_resumed_two_blocks"] = Case(leaf, [BAI_MAX + 1 + G30], isize=sizes_to(sum(len(r) for r in leaf[:4]), n))
    # 6. the other ends of min_shift
    for sh in (10, 24):
        c["shift_%d" % sh] = Case([m(0, 3, b"a"), m(0, (1 << sh) - 1, b"last"), m(0, 1 << sh, b"first"), m(0, (1 << sh) + 7, b"next"), m(0, TOP - 10, b"end")], [TOP], sh, hdr=33)
    c["shift_10_short_contig"] = Case([m(0, 1023, b"last"), m(0, 1024, b"first"), m(0, 4000, b"far", "500M")], [5000], 10, hdr=33)
    c["shift_0_means_14"] = Case(few(TOP), [TOP], 0, hdr=31)
    # 7. counts
    c["placed_unmapped"] = Case([m(0, G30 + 10, b"map"), rec(0, G30 + 10, b"un", flag=4 | 1 | 8), m(0, G30 + 20, b"unc", "50M", flag=4), rec(1, 16383, b"un2", flag=4),
                                 m(1, 16383, b"mate2", "2M"), rec(-1, -1, b"un3", flag=4)], [TOP, 16385], hdr=12)
    c["only_unplaced"] = Case([rec(-1, -1, b"u%d" % k, l_seq=k) for k in range(5)], [TOP, 2000])
    c["empty_contigs"] = Case([m(1, 5, b"a"), m(1, G30 + 9, b"b"), m(3, 0, b"c")], [100, TOP, 300, TOP, 500], hdr=12)
    c["empty"] = Case([], [TOP, 2000], isize=[], eof=0)
    c["header_only"] = Case([], [TOP], hdr=40)
    # 8. baicases' cuts, the records above 2^30
    body = [m(0, G30 + 10 + k, b"b%d" % k, l_seq=k % 5) for k in range(12)]
    off = [0]
    for r in body:
        off.append(off[-1] + len(r))
    n = off[-1]
    c["block_size_cut"] = Case(body, [TOP], isize=sizes_to(off[3] + 1, off[5] + 2, off[8] + 3, n), slabs=(1, 150, 250))
    r = m(0, G30 + 50, b"somename", "3M2I4M1D5M", l_seq=14)
    pre = [m(0, G30 + 40, b"p")]
    q = len(pre[0])
    for name, cut in (("slab_cuts_fixed", q + 20), ("slab_cuts_name", q + 36 + 4), ("slab_cuts_cigar", q + 36 + 9 + 6), ("slab_cuts_between", q)):
        tail = [m(0, G30 + 60, b"t")]
        c[name] = Case(pre + [r] + tail, [TOP], isize=sizes_to(cut, q + len(r) + len(tail[0])), slabs=(1, 1, 1))
    long_cig = "".join("%dM%dI" % (1 + k % 3, 1 + k % 2) for k in range(200))
    c["longer_than_a_slab"] = Case([m(0, G30 + 3, b"a"), m(0, G30 + 4, b"long", long_cig, l_seq=900), m(0, G30 + 4, b"b"), m(1, 0, b"c")], [TOP, 100], slabs=(113, 400, 1000))
    # 9. refusals
    good = [m(0, G30 + 10 + k, b"g%d" % k) for k in range(8)]
    g = [0]
    for x in good:
        g.append(g[-1] + len(x))
    early = m(0, G30 + 3, b"early")
    for sh in (9, 25, -1):
        c["refuse_shift_%d" % sh] = Case(good, [TOP], sh)
    c["refuse_order"] = Case(good[:5] + [early] + good[5:], [TOP])
    c["refuse_order_at_slab_border"] = Case(good[:4] + [early] + good[4:], [TOP], isize=sizes_to(g[4], g[-1] + len(early)), slabs=(1, g[4], g[4] + 1))
    c["refuse_refid_n_ref"] = Case(good + [m(1, 0, b"r")], [TOP])
    c["refuse_refid_minus_2"] = Case(good + [m(-2, 0, b"r")], [TOP])
    c["refuse_negative_pos"] = Case([m(0, -1, b"n")] + good, [TOP])
    c["refuse_end_beyond_contig"] = Case(good + [m(0, TOP - 5, b"e", "6M")], [TOP])
    return c


def regions(case):
    """what check_cases and the GPU test ask of an accepted case: around every record and every level border it lies next to, and whole contigs"""
    out = [(i, 0, l) for i, l in enumerate(case.ref_len)]
    for r in case.recs[::max(1, len(case.recs) // 20)]:          # (the cases of hundreds of like records: a twentieth of them)
        rid = fields(r)[1]
        if rid < 0:
            continue
        beg, end = interval(r)
        top = case.ref_len[rid]
        for a, b in ((beg, beg + 1), (end - 1, end), (end, end + 1), (beg - 1, beg), (beg + 3, end + 40000), (beg - 20000, beg + 2), ((beg >> 14) << 14, ((beg >> 14) + 1) << 14)):
            a, b = max(a, 0), min(b, top)
            if a < b:
                out.append((rid, a, b))
    return out


def check_cases():
    bc.check_cases()
    c = cases()
    # the formulas, once each
    assert [meta_bin(d) for d in (5, 6, 7)] == [37450, 299594, 2396746] and [first_bin(l) for l in range(7)] == [0, 1, 9, 73, 585, 4681, 37449]
    assert scheme(14, [BAI_MAX]) == (14, 5) and scheme(14, [BAI_MAX + 1]) == (14, 6) and scheme(14, [TOP]) == (14, 6) and scheme(0, [7]) == (14, 5)
    assert scheme(12, [TOP]) == (12, 7) and scheme(16, [TOP]) == (16, 5) and scheme(10, [TOP]) == (10, 7) and scheme(24, [TOP]) == (24, 5)
    assert max(reg2bins(0, TOP, 10, 7)) < 1 << 22
    for beg, end in ((0, 1), (16383, 16385), (16384, 16385), (1 << 26, (1 << 26) + 1), ((1 << 26) - 1, (1 << 26) + 1), (BAI_MAX - 1, BAI_MAX), (12345678, 12345999), (0, BAI_MAX)):
        assert reg2bin(beg, end, 14, 5) == bc.reg2bin(beg, end) and reg2bins(beg, end, 14, 5) == bc.reg2bins(beg, end)
    for name, k in c.items():
        keys = [(fields(r)[1] & 0xFFFFFFFF, fields(r)[2]) for r in k.recs]
        assert (keys == sorted(keys)) == (not name.startswith("refuse_order")), name
        assert (k.refused is not None) == name.startswith("refuse_"), name
        assert len(k.slabs) == 4 and k.slabs[-1] == 0
    # 1. inherited
    leaves = 0
    for name, k in bc.cases().items():
        if k.refused is None:
            leaves += same_as_bai(c["bai_" + name].want, k.want)
    assert leaves > 300 and all("bai_" + n in c for n in INHERITED_BAI)
    # 2. depth
    hd = lambda n: (read_csi(c[n].want)["min_shift"], read_csi(c[n].want)["depth"], max(c[n].ref_len))
    assert hd("depth5_at_2_29") == (14, 5, BAI_MAX) and hd("depth6_at_2_29_plus_1") == (14, 6, BAI_MAX + 1) and hd("depth6_at_2_31_minus_1") == (14, 6, TOP)
    assert hd("depth7_at_shift_12") == (12, 7, TOP) and hd("depth5_at_shift_16") == (16, 5, TOP) and hd("shift_0_means_14") == (14, 6, TOP)
    assert struct.pack("<I", 2396746) in c["depth7_at_shift_12"].want and struct.pack("<I", 37450) in c["depth5_at_shift_16"].want
    assert interval(c["depth6_at_2_31_minus_1"].recs[-1])[1] == TOP and same_as_bai(c["depth5_at_2_29"].want, c["depth5_at_2_29"].bai) == 3
    # 3. level borders at depth 6: leaves from 37449 on, a level up across a border, bin 0 across 2^29
    k = c["level_borders_depth6"]
    lb = {fields(r)[2]: reg2bin(*interval(r), 14, 6) for r in k.recs}
    for sh, parent in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1), (29, 0)):
        assert lb[(1 << sh) - 10] == 37449 + (((1 << sh) - 10) >> 14) and lb[1 << sh] == 37449 + (1 << sh >> 14)
        assert lb[(1 << sh) - 5] == parent + (((1 << sh) - 5) >> (sh + 3) if parent else 0)
    assert lb[BAI_MAX - 5] == 0 and lb[BAI_MAX + 1000] == 2 and BAI_MAX < interval(k.recs[-1])[1] < G30
    assert sorted(read_csi(k.want)["refs"][0]["bins"]) == sorted(set(lb.values()))
    # 4. bins 65,536 apart
    k = c["bins_65536_apart"]
    b1, b2 = (reg2bin(*interval(r), 14, 6) for r in k.recs[1:3])
    assert b2 - b1 == 65536 and fields(k.recs[2])[2] - fields(k.recs[1])[2] == G30 and {b1, b2} <= set(read_csi(k.want)["refs"][0]["bins"])
    k = c["bins_65536_apart_two_contigs"]
    b0, b1 = (reg2bin(*interval(r), 14, 6) for r in k.recs[1:3])
    assert b0 == b1 + 65536 and (0 << 16 | b0) == (1 << 16 | b1) and [fields(r)[1] for r in k.recs[1:3]] == [0, 1]
    two = read_csi(k.want)["refs"]
    assert b0 in two[0]["bins"] and b1 in two[1]["bins"] and b1 not in two[0]["bins"]
    # 5. loffset
    k = c["loffset_backfilled"]
    x = read_csi(k.want)["refs"][0]
    b = reg2bin(*interval(k.recs[1]), 14, 6)
    V = voffsets(k.at, k.isize)[0]
    assert level_of(b) == 5 and first_window(b, 6) == (interval(k.recs[1])[0] >> 14) - 3 and x["loff"][b] == V(k.off[1]) == x["bins"][b][0][0] > 0
    k = c["loffset_parent_first"]
    x = read_csi(k.want)["refs"][0]
    parent, leaf = reg2bin(*interval(k.recs[1]), 14, 6), reg2bin(*interval(k.recs[2]), 14, 6)
    V = voffsets(k.at, k.isize)[0]
    assert level_of(parent) == 5 and level_of(leaf) == 6 and (leaf - 1) >> 3 == parent
    assert x["loff"][leaf] == x["loff"][parent] == V(k.off[1]) < x["bins"][leaf][0][0] == V(k.off[2])        # the leaf's bound is the parent's record
    k = c["loffset_unset_windows"]
    x = read_csi(k.want)["refs"][0]
    V = voffsets(k.at, k.isize)[0]
    far = reg2bin(*interval(k.recs[4]), 14, 6)
    assert first_window(far, 6) == 65536 + 40 and x["loff"][far] == V(k.off[4]) and x["loff"][reg2bin(*interval(k.recs[3]), 14, 6)] == V(k.off[3])
    one, two = read_csi(c["leaf_resumed_one_block"].want)["refs"][0]["bins"], read_csi(c["leaf_resumed_two_blocks"].want)["refs"][0]["bins"]
    lf = 37449 + ((G30 + 20000) >> 14)
    assert sorted(one) == sorted(two) == sorted([37449, (lf - 1) >> 3, lf]) and len(one[lf]) == 1 and len(two[lf]) == 2     # joined in one block, apart in two
    # 6. min_shift 10 and 24
    for sh, depth in ((10, 7), (24, 5)):
        k = c["shift_%d" % sh]
        x = read_csi(k.want)
        assert (x["min_shift"], x["depth"]) == (sh, depth) and [fields(r)[2] for r in k.recs[1:3]] == [(1 << sh) - 1, 1 << sh]
        assert [reg2bin(*interval(r), sh, depth) for r in k.recs[1:3]] == [first_bin(depth - 1), first_bin(depth) + 1]       # across the first window's end, and the second window
    assert hd("shift_10_short_contig") == (10, 5, 5000)
    # 7. counts
    x = read_csi(c["placed_unmapped"].want)
    assert [r["meta"][1] for r in x["refs"]] == [(1, 2), (1, 1)] and x["n_no_coor"] == 1
    assert read_csi(c["only_unplaced"].want) == dict(min_shift=14, depth=6, refs=[dict(bins={}, loff={}, meta=None)] * 2, n_no_coor=5)
    assert [bool(r["bins"]) for r in read_csi(c["empty_contigs"].want)["refs"]] == [False, True, False, True, False]
    assert c["empty"].stream == b"" and c["empty"].isize == [] and len(c["empty"].want) == 20 + 2 * 4 + 8 and len(c["header_only"].want) == 20 + 4 + 8
    # 8. cuts
    bcut = c["block_size_cut"]
    assert [min(x - o for o in bcut.off if o <= x) for x in bcut.cuts()[:3]] == [1, 2, 3]
    r0 = c["slab_cuts_fixed"].off[1]
    assert c["slab_cuts_fixed"].cuts()[0] - r0 == 20 and c["slab_cuts_name"].cuts()[0] - r0 == 40 and c["slab_cuts_cigar"].cuts()[0] - r0 == 36 + 9 + 6
    assert c["slab_cuts_between"].cuts()[0] == r0
    lg = c["longer_than_a_slab"]
    assert 36 + 5 + 4 * fields(lg.recs[1])[4] > max(lg.slabs) and len(lg.recs[1]) > 2 * max(lg.slabs)
    for n in ("block_size_cut", "slab_cuts_fixed", "slab_cuts_name", "slab_cuts_cigar", "slab_cuts_between", "longer_than_a_slab"):
        assert max(c[n].ref_len) == TOP and all(fields(r)[2] > G30 for r in c[n].recs if fields(r)[1] == 0)
    # 9. refusals
    for sh in (9, 25, -1):
        e = c["refuse_shift_%d" % sh].refused
        assert e.code == ARX_E_ARG and e.record is None
    for name, rule, record in (("refuse_order", R_ORDER, 5), ("refuse_order_at_slab_border", R_ORDER, 4), ("refuse_refid_n_ref", R_REFID, 8), ("refuse_refid_minus_2", R_REFID, 8),
                               ("refuse_negative_pos", R_POS, 0), ("refuse_end_beyond_contig", R_END, 8)):
        e = c[name].refused
        assert (e.code, e.rule, e.record) == (ARX_E_ARG, rule, record), (name, e)
    sb = c["refuse_order_at_slab_border"]
    assert sb.cuts()[0] == sb.off[4] and sb.slabs[1] == sb.isize[0]
    assert interval(c["refuse_end_beyond_contig"].recs[-1])[1] == TOP + 1
    # the reader over every accepted case, against brute force
    bounds, hits = [], 0
    for name, k in c.items():
        if k.refused is not None:
            continue
        csi, reader = read_csi(k.want), StreamReader(k)
        placed = sum(sum(r["meta"][1]) for r in csi["refs"] if r["meta"])
        assert placed + csi["n_no_coor"] == len(k.recs), name
        for rid, beg, end in regions(k):
            got = query(csi, reader, rid, beg, end, bounds)
            assert got == bc.brute(k.recs, rid, beg, end), (name, rid, beg, end)
            hits += len(got)
    assert len(bounds) > 1000 and hits > len(bounds) and 4 * sum(1 for b in bounds if b > 0) >= len(bounds), (len(bounds), sum(1 for b in bounds if b > 0))
    return len(bounds), sum(1 for b in bounds if b > 0)

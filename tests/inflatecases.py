"""The block cases of the device inflate, shared by the host program (test_inflate_sim.py) and the GPU test (test_inflate_gpu.py): chains of
BGZF blocks with what they must inflate to.  The expected bytes come from Python's zlib; the structure of a stream (how many DEFLATE blocks,
which code lengths, whether a code-length run crosses from the literal/length lengths into the distance lengths) comes from scan() below, a
plain RFC 1951 decoder whose output is checked against zlib's on every valid block.  Neither is code under test.

Streams zlib never writes (a block without a distance code, the one-code distance set, a run across the two sets of lengths, an invalid
symbol, a distance before the start) are written bit by bit with dynamic_block() / fixed_block()."""
import collections
import struct
import zlib

import numpy as np

import bgzfio

OK, BAD_HEADER, BAD_BTYPE, BAD_STORED_LEN, BAD_CODE_LENGTHS, BAD_SYMBOL, BAD_DISTANCE, TRUNCATED, SIZE_MISMATCH, CRC_MISMATCH = range(10)
ARX_OK, ARX_E_ARG, ARX_E_IO = 0, -2, -5

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


# ---- reading: a plain decoder that reports the structure of a stream
class _Reader:
    def __init__(self, data):
        self.d, self.at, self.buf, self.n = data, 0, 0, 0

    def peek(self, k):
        while self.n < k and self.at < len(self.d):
            self.buf |= self.d[self.at] << self.n
            self.at += 1
            self.n += 8
        return self.buf & ((1 << k) - 1)

    def drop(self, k):
        if k > self.n:
            raise ValueError("truncated")
        self.buf >>= k
        self.n -= k

    def get(self, k):
        v = self.peek(k)
        self.drop(k)
        return v

    def bitpos(self):
        return 8 * self.at - self.n


def canonical(lens):
    """code lengths -> the canonical codes (RFC 1951 3.2.2), None for unused symbols"""
    count = collections.Counter(l for l in lens if l)
    code, nxt = 0, {}
    for l in range(1, 16):
        code = (code + count.get(l - 1, 0)) << 1
        nxt[l] = code
    out = []
    for l in lens:
        if l:
            out.append(nxt[l])
            nxt[l] += 1
        else:
            out.append(None)
    return out


def _rev(c, n):
    return int(format(c, "0%db" % n)[::-1], 2)


def _table(lens):
    top = max(lens) if any(lens) else 0
    tab = [None] * (1 << top)
    for s, (l, c) in enumerate(zip(lens, canonical(lens))):
        if l:
            for k in range(_rev(c, l), 1 << top, 1 << l):
                tab[k] = (s, l)
    return tab, top


def _sym(r, tab, top):
    e = tab[r.peek(top)] if top else None
    if e is None:
        raise ValueError("no such code")
    r.drop(e[1])
    return e[0]


def scan(payload):
    """a valid raw DEFLATE stream -> (its bytes, [one dict per DEFLATE block: btype, bitpos, and for btype 2 hlit, hdist, hclen, ll_lens,
    d_lens, crossing (a 16/17/18 run that starts in the literal/length lengths and ends in the distance lengths), for btype 1 and 2 max_dist,
    n_matches and ends_in_match (the token in front of the end-of-block symbol is a match)])"""
    r, out, blocks = _Reader(payload), bytearray(), []
    while True:
        b = dict(bitpos=r.bitpos())
        final, b["btype"] = r.get(1), r.get(2)
        blocks.append(b)
        if b["btype"] == 0:
            r.drop(r.n & 7)
            n, nn = r.get(16), r.get(16)
            assert n ^ 0xFFFF == nn and r.n % 8 == 0
            r.at, r.buf, r.n = r.at - r.n // 8, 0, 0          # bytes read ahead go back
            out += r.d[r.at:r.at + n]
            assert r.at + n <= len(r.d)
            r.at += n
        else:
            assert b["btype"] in (1, 2)
            ll, dl = FIXED_LL, FIXED_D
            if b["btype"] == 2:
                hlit, hdist, hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = r.get(3)
                tab, top = _table(cl)
                lens, crossing = [], False
                while len(lens) < hlit + hdist:
                    s = _sym(r, tab, top)
                    if s < 16:
                        lens.append(s)
                        continue
                    rep, val = (3 + r.get(2), lens[-1]) if s == 16 else (3 + r.get(3), 0) if s == 17 else (11 + r.get(7), 0)
                    crossing |= len(lens) < hlit < len(lens) + rep
                    lens += [val] * rep
                assert len(lens) == hlit + hdist
                ll, dl = lens[:hlit], lens[hlit:]
                b.update(hlit=hlit, hdist=hdist, hclen=hclen, ll_lens=ll, d_lens=dl, crossing=crossing)
            (lt, ltop), (dt, dtop) = _table(ll), _table(dl)
            b.update(max_dist=0, n_matches=0, ends_in_match=False)
            while True:
                s = _sym(r, lt, ltop)
                if s < 256:
                    out.append(s)
                    b["ends_in_match"] = False
                elif s == 256:
                    break
                else:
                    n = LBASE[s - 257] + r.get(LEXT[s - 257])
                    ds = _sym(r, dt, dtop)
                    dist = DBASE[ds] + r.get(DEXT[ds])
                    assert dist <= len(out)
                    b["max_dist"], b["n_matches"], b["ends_in_match"] = max(b["max_dist"], dist), b["n_matches"] + 1, True
                    for _ in range(n):
                        out.append(out[-dist])
        if final:
            return bytes(out), blocks


# ---- writing, bit by bit
class BitWriter:
    def __init__(self):
        self.buf, self.n = 0, 0

    def put(self, v, k):
        """k bits of v, least significant first (header fields, extra bits)"""
        self.buf |= (v & ((1 << k) - 1)) << self.n
        self.n += k

    def code(self, c, k):
        """a Huffman code: most significant bit first"""
        self.put(_rev(c, k), k)

    def bytes(self):
        return self.buf.to_bytes((self.n + 7) // 8, "little")


def _tokens(w, tokens, ll_lens, d_lens):
    lc, dc = canonical(ll_lens), canonical(d_lens)
    for t in tokens:
        if isinstance(t, tuple) and t[0] == "sym":          # a raw literal/length symbol, valid or not
            w.code(lc[t[1]], ll_lens[t[1]])
        elif isinstance(t, tuple) and t[0] == "dsym":       # a raw distance symbol
            w.code(dc[t[1]], d_lens[t[1]])
        elif isinstance(t, tuple):
            n, dist = t
            ls = max(i for i in range(29) if LBASE[i] <= n) if n < 258 else 28
            ds = max(i for i in range(30) if DBASE[i] <= dist)
            w.code(lc[257 + ls], ll_lens[257 + ls])
            w.put(n - LBASE[ls], LEXT[ls])
            w.code(dc[ds], d_lens[ds])
            w.put(dist - DBASE[ds], DEXT[ds])
        else:
            w.code(lc[t], ll_lens[t])
    w.code(lc[256], ll_lens[256])


def stored_block(data, final=False, w=None):
    w = w or BitWriter()
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.put(0, -w.n % 8)
    w.put(len(data), 16)
    w.put(len(data) ^ 0xFFFF, 16)
    for x in data:
        w.put(x, 8)
    return w


def fixed_block(tokens, final=True, w=None):
    """tokens: a byte value, (length, distance), ("sym", s) or ("dsym", s); the end-of-block symbol is added"""
    w = w or BitWriter()
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    _tokens(w, tokens, FIXED_LL, FIXED_D)
    return w


def dynamic_block(tokens, ll_lens, d_lens, final=True, w=None, length_codes=None):
    """a BTYPE 2 block with the given code lengths (len(ll_lens) = HLIT >= 257, len(d_lens) = HDIST >= 1).  The lengths go out as ONE sequence:
    runs of three and more zeros as 17 / 18, wherever they lie -- across the border between the two sets too -- everything else literally.
    The code length code is a fixed complete one: 4 bits for 0..12, 5 bits for 13..18"""
    w = w or BitWriter()
    cl = [4] * 13 + [5] * 6
    cc = canonical(cl)
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(len(ll_lens) - 257, 5)
    w.put(len(d_lens) - 1, 5)
    w.put(15, 4)
    for s in CL_ORDER:
        w.put(cl[s], 3)
    seq, i = list(ll_lens) + list(d_lens), 0
    if length_codes is not None:                             # the code length symbols as given, (symbol, extra value): valid or not
        for sym, extra in length_codes:
            w.code(cc[sym], cl[sym])
            w.put(extra, {16: 2, 17: 3, 18: 7}.get(sym, 0))
        i = len(seq)
    while i < len(seq):
        run = 0
        while i + run < len(seq) and seq[i + run] == 0 and run < 138:
            run += 1
        if run >= 11:
            w.code(cc[18], cl[18]); w.put(run - 11, 7); i += run
        elif run >= 3:
            w.code(cc[17], cl[17]); w.put(run - 3, 3); i += run
        else:
            w.code(cc[seq[i]], cl[seq[i]]); i += 1
    _tokens(w, tokens, ll_lens, d_lens)
    return w


# ---- inputs
def fastq_text(n, seed):
    rng = np.random.default_rng(seed)
    out = bytearray()
    k = 0
    while len(out) < n:
        seq = bytes(b"ACGT"[i] for i in rng.integers(0, 4, 150))
        qual = bytes(int(q) for q in np.array([35, 45, 56, 70], np.uint8)[rng.choice(4, 150, p=[.02, .05, .13, .8])])
        out += b"@A00519:77:H7:1:%d:%d:%d BX:Z:A%02dC%02dB%02dD%02d\n" % (1101 + k // 50, int(rng.integers(1000, 30000)), int(rng.integers(1000, 30000)),
                                                                        k // 40 % 96, k // 7 % 96, k % 96, k // 3 % 96) + seq + b"\n+\n" + qual + b"\n"
        k += 1
    return bytes(out[:n])


def fibonacci_bytes(seed=5):
    f = [1, 1]
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    v = np.concatenate([np.full(c, 65 + i, np.uint8) for i, c in enumerate(f)])
    np.random.default_rng(seed).shuffle(v)
    return v.tobytes()                                        # 46367 bytes


Case = collections.namedtuple("Case", "chain status data n_deflate ret")
# chain: the bytes handed in; status: per block; data: per block the bytes it inflates to (None for a bad block); n_deflate: DEFLATE blocks
# in the whole chain (None where a block is bad: how far a damaged stream is read is not pinned); ret: the entry's return value


def _good(chain):
    data, nd = [], 0
    for b in bgzfio.split(chain):
        d = zlib.decompress(b["payload"], -15)
        assert len(d) == b["isize"] and zlib.crc32(d) == b["crc"]
        got, blocks = scan(b["payload"])
        assert got == d                                       # the scanner reads what zlib reads
        data.append(d)
        nd += len(blocks)
    return Case(chain, [OK] * len(data), data, nd, ARX_OK)


def _raw_block(payload, data, **kw):
    return bgzfio.frame(payload, zlib.crc32(data), len(data), **kw)


def handmade_streams():
    """name -> (payload, bytes): the dynamic blocks zlib does not write"""
    out = {}
    lits = list(b"abcdefghijklmno")
    # no match at all: HDIST = 1 and that one length 0
    ll = [0] * 257
    for s in lits + [256]:
        ll[s] = 4
    toks = [lits[i * 7 % 15] for i in range(400)]
    out["no_distance_code"] = (dynamic_block(toks, ll, [0]).bytes(), bytes(toks))
    # matches through a single distance code of one bit: the incomplete set zlib's inflate accepts
    ll = [0] * 258
    for s in lits[:14] + [256, 257]:
        ll[s] = 4
    toks, data = [], bytearray()
    for i in range(300):
        if i % 5 == 4:
            toks.append((3, 3)); data += bytes(data[-3 + k] for k in range(3))
        else:
            toks.append(lits[i * 3 % 14]); data.append(lits[i * 3 % 14])
    out["single_distance_code"] = (dynamic_block(toks, ll, [0, 0, 1]).bytes(), bytes(data))
    # a run of zeros from the literal/length lengths into the distance lengths: HLIT = 270 with 259..269 unused, distance codes 9 and 10 only
    ll = [0] * 270
    for s in lits[:13] + [256, 257, 258]:
        ll[s] = 4
    toks, data = [], bytearray()
    for i in range(300):
        if i > 60 and i % 6 == 0:
            n, dist = (3, 25 + i % 8) if i % 12 else (4, 33 + i % 16)
            toks.append((n, dist)); data += bytes(data[-dist + k] for k in range(n))
        else:
            toks.append(lits[i * 5 % 13]); data.append(lits[i * 5 % 13])
    out["run_across_the_border"] = (dynamic_block(toks, ll, [0] * 9 + [1, 1]).bytes(), bytes(data))
    return out


_CACHE = {}


def good_cases():
    """name -> Case, every block valid.  Built once per process"""
    if "good" in _CACHE:
        return _CACHE["good"]
    rng = np.random.default_rng(31)
    text = fastq_text(bgzfio.BLOCK_IN, 1)
    c = {}
    # 1. stored
    c["stored_level0"] = bgzfio.write_bgzf(text[:1000], level=0, eof=False) + bgzfio.write_bgzf(text[:65000], level=0, eof=False)
    c["stored_empty"] = _raw_block(bytes.fromhex("010000ffff"), b"")
    for n in (1, 2, 65280, 65536):                           # 65536 incompressible bytes do not fit one block (BSIZE): they are cut at 65280
        c["stored_random_%d" % n] = bgzfio.write_bgzf(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), eof=False)
    c["full_block_65536"] = bgzfio.block(fastq_text(65536, 2), 4)   # the largest ISIZE there is
    # 2. the fixed code
    c["fixed_text"] = bgzfio.block(text[:3000], 6, 8, zlib.Z_FIXED)
    c["fixed_few_bytes"] = b"".join(bgzfio.block(text[:n]) for n in (1, 3, 4, 9))
    # 3. dynamic codes
    for level in (1, 4, 6, 9):
        c["dynamic_level%d" % level] = bgzfio.block(text, level)
    c["dynamic_memlevel1"] = bgzfio.block(text, 6, 1)
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    pieces = z.compress(text[:777]) + z.flush(zlib.Z_SYNC_FLUSH) + z.compress(text[777:3000]) + z.flush(zlib.Z_FULL_FLUSH) + z.compress(text[3000:3001]) + \
        z.flush(zlib.Z_SYNC_FLUSH) + z.compress(text[3001:9000]) + z.flush()
    c["dynamic_flushes"] = _raw_block(pieces, text[:9000])
    # 4. matches
    c["run_of_one_byte"] = bgzfio.block(b"a" * 65280, 9)
    for p in (2, 3, 7):
        c["period_%d" % p] = bgzfio.block((b"abcdefg"[:p] * 65280)[:65280], 6)
    # zlib never looks back more than 32,506 bytes, so the window's edge is written by hand: 32,768 stored bytes, then matches of 258 and of
    # 3 bytes at distance 32,768 (distance symbol 29 with all 13 extra bits set)
    a = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    far = a + a[:261]
    c["distance_32768"] = _raw_block(fixed_block([(258, 32768), (3, 32768)], w=stored_block(a)).bytes(), far)
    c["match_ends_on_last_byte"] = bgzfio.block(text[:5000] + text[100:140], 9)
    # 5. codes
    c["fifteen_bit_codes"] = bgzfio.block(fibonacci_bytes(), 6, 9, zlib.Z_HUFFMAN_ONLY)
    for name, (payload, data) in handmade_streams().items():
        c[name] = _raw_block(payload, data)
    # 6. framing
    small = bgzfio.block(text[:300])
    c["isize_0_in_the_middle_and_at_the_end"] = small + bgzfio.EOF_BLOCK + bgzfio.block(text[300:900]) + bgzfio.EOF_BLOCK
    c["isize_1"] = bgzfio.block(b"@") + small
    c["extra_subfield_in_front_of_bc"] = bgzfio.block(text[:500], extra_front=b"XY" + struct.pack("<H", 3) + b"abc") + small
    sizes = rng.integers(0, 2001, 300)
    long_text = fastq_text(int(sizes.sum()), 3)
    c["three_hundred_blocks"] = bgzfio.write_bgzf(long_text, cut=np.cumsum(sizes)[:-1].tolist(), level=4, eof=False)
    _CACHE["good"] = {k: _good(v) for k, v in c.items()}
    return _CACHE["good"]


def structure(name):
    """the DEFLATE blocks (scan's dicts) of case `name`'s first BGZF block"""
    return scan(bgzfio.split(good_cases()[name].chain)[0]["payload"])[1]


def _patch_bits(payload, bitpos, k, value):
    v = int.from_bytes(payload, "little")
    v = v & ~(((1 << k) - 1) << bitpos) | value << bitpos
    return v.to_bytes(len(payload), "little")


def damage_cases():
    """name -> Case: one damaged block between two good ones; the entry returns ARX_E_IO"""
    if "damage" in _CACHE:
        return _CACHE["damage"]
    text = fastq_text(6000, 4)
    front, back = text[:700], text[5000:5600]
    mid = text[1000:4000]
    dyn = bgzfio.deflate_raw(mid, 6)
    assert dyn[0] & 7 == 5                                    # one final dynamic block
    stored = bgzfio.deflate_raw(mid[:200], 0)
    crc, n = zlib.crc32(mid), len(mid)
    bad = {}
    bad["truncated"] = (bgzfio.frame(dyn[:len(dyn) // 2], crc, n), TRUNCATED)
    bad["truncated_in_the_code_lengths"] = (bgzfio.frame(dyn[:20], crc, n), TRUNCATED)
    bad["truncated_empty"] = (bgzfio.frame(b"", crc, n), TRUNCATED)
    bad["btype_3"] = (bgzfio.frame(bytes([dyn[0] | 6]) + dyn[1:], crc, n), BAD_BTYPE)
    bad["stored_nlen"] = (bgzfio.frame(stored[:3] + bytes([stored[3] ^ 0x10]) + stored[4:], zlib.crc32(mid[:200]), 200), BAD_STORED_LEN)
    # a code length code of one bit more than the complete set holds: over-subscribed.  The 3-bit lengths start at bit 17
    cl = [int.from_bytes(dyn[:16], "little") >> (17 + 3 * i) & 7 for i in range((dyn[1] >> 5 | (dyn[2] & 1) << 3) + 4)]
    k = next(i for i, l in enumerate(cl) if l != 1)
    bad["code_lengths_over_subscribed"] = (bgzfio.frame(_patch_bits(dyn, 17 + 3 * k, 3, 1), crc, n), BAD_CODE_LENGTHS)
    lits = list(b"abcdefghijklmno")
    ll = [0] * 257
    for s in lits + [256]:
        ll[s] = 4
    toks = [lits[i % 15] for i in range(100)]
    inc = list(ll)
    inc[lits[0]] = 5                                          # an incomplete literal/length set
    bad["code_lengths_incomplete"] = (_raw_block(dynamic_block(toks[1:], inc, [0]).bytes() + b"\0" * 4, bytes(toks[1:])), BAD_CODE_LENGTHS)
    bad["two_distance_codes_incomplete"] = (_raw_block(dynamic_block(toks, ll, [2, 2]).bytes() + b"\0" * 4, bytes(toks)), BAD_CODE_LENGTHS)
    direct = [(l, 0) for l in ll]
    bad["repeat_without_a_previous_length"] = (_raw_block(dynamic_block(toks, ll, [0], length_codes=[(16, 0)] + direct[3:] + [(0, 0)]).bytes() + b"\0" * 4, bytes(toks)),
                                               BAD_CODE_LENGTHS)
    bad["repeat_past_the_last_length"] = (_raw_block(dynamic_block(toks, ll, [0], length_codes=direct + [(18, 127)]).bytes() + b"\0" * 4, bytes(toks)), BAD_CODE_LENGTHS)
    bad["hlit_287"] = (bgzfio.frame(_patch_bits(dyn, 3, 5, 30), crc, n), BAD_CODE_LENGTHS)
    head = list(b"arachne ") * 4
    bad["symbol_286"] = (_raw_block(fixed_block(head + [("sym", 286)] + head).bytes() + b"\0" * 4, bytes(head)), BAD_SYMBOL)
    bad["distance_symbol_30"] = (_raw_block(fixed_block(head + [("sym", 257), ("dsym", 30)] + head).bytes() + b"\0" * 4, bytes(head)), BAD_SYMBOL)
    ll2 = [0] * 258
    for s in lits[:14] + [256, 257]:
        ll2[s] = 4
    toks2 = [lits[i % 14] for i in range(100)]
    bad["length_without_a_distance_code"] = (_raw_block(dynamic_block(toks2 + [("sym", 257)] + toks2, ll2, [0]).bytes() + b"\0" * 4, bytes(toks2)), BAD_SYMBOL)
    bad["distance_before_the_start"] = (_raw_block(fixed_block(head[:5] + [(3, 6)] + head).bytes(), bytes(head)), BAD_DISTANCE)
    bad["isize_up"] = (bgzfio.frame(dyn, crc, n + 1), SIZE_MISMATCH)
    bad["isize_down"] = (bgzfio.frame(dyn, crc, n - 1), SIZE_MISMATCH)
    bad["crc"] = (bgzfio.frame(dyn, crc ^ 1, n), CRC_MISMATCH)
    bad["header_cm_7"] = (bgzfio.frame(dyn, crc, n, cm=7), BAD_HEADER)
    bad["header_fname_flag"] = (bgzfio.frame(dyn, crc, n, flg=12), BAD_HEADER)
    bad["header_isize_70000"] = (bgzfio.frame(dyn, crc, 70000), BAD_HEADER)
    a, b = bgzfio.block(front, 6), bgzfio.block(back, 1)
    out = {}
    for name, (blk, st) in bad.items():
        out[name] = Case(a + blk + b, [OK, st, OK], [front, None, back], None, ARX_E_IO)
    _CACHE["damage"] = out
    return out


def untiled_chains():
    """chains whose headers do not tile the bytes: the entry returns ARX_E_ARG"""
    text = fastq_text(2000, 6)
    a, b = bgzfio.block(text[:900]), bgzfio.block(text[900:])
    return {"bsize_overruns": a + b[:-5], "no_magic": a + b"\0" + b, "no_bc_subfield": a + b[:12] + b"XC" + b[14:], "header_cut": a + b[:10]}


def block_offsets(chain):
    """[(output offset, isize as the walk counts it)] per block: a block whose header is refused counts as empty"""
    out, at = [], 0
    for blk in bgzfio.split(chain):
        raw = chain[blk["at"]:blk["at"] + blk["size"]]
        sound = raw[2] == 8 and raw[3] == 4 and blk["isize"] <= 65536
        n = blk["isize"] if sound else 0
        out.append((at, n))
        at += n
    return out

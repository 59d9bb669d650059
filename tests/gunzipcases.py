"""The cases of the chunked gzip inflate (arachne_amd/csrc/dev_gunzip.h, gunzip_host.h), shared by the host program (test_gunzip_sim.py) and the
GPU test (test_gunzip_gpu.py): whole gzip files with the sizes they are read with and what must come of them.  The expected bytes come from
readers that are not under test: Python's zlib.decompressobj(31), member by member, under gzread's rule for what follows a member (expected()
below), and gzread itself inside the host program.  The streams are written with zlib / gzip and, where zlib writes no such stream, bit by bit
with inflatecases.py's stored_block / fixed_block / dynamic_block."""
import collections
import os
import struct
import subprocess
import zlib

import numpy as np

import inflatecases as ic

ARX_OK, ARX_E_ARG, ARX_E_IO = 0, -2, -5
FB_NONE, FB_REFUTED, FB_OVERFLOW, FB_STATUS, FB_CHECK, FB_NO_BLOCK, FB_CUT_SHORT = range(7)

Case = collections.namedtuple("Case", "data chunk slab expand clean reason ret")
# data: the file; chunk, slab, expand: arx_selftest_gunzip's chunk_bytes, slab_bytes and expand; clean: the device must take all of it
# (stats[10] == 0 and stats[11] == 0); reason: stats[11] where the host must take over (None: not pinned); ret: the entry's return value


def expected(data):
    """what gzread reads from the file -> (bytes, members, bytes ignored behind the last member), or None where it reports an error"""
    out, members, at = bytearray(), 0, 0
    while at < len(data):
        rest = data[at:]
        if rest[:2] != b"\x1f\x8b":
            if members == 0:
                return bytes(rest), 0, 0                     # no gzip file: handed on as it is
            return bytes(out), members, len(rest)
        d = zlib.decompressobj(31)
        try:
            out += d.decompress(rest)
        except zlib.error:
            return None
        if not d.eof:
            return None
        at = len(data) - len(d.unused_data)
        members += 1
    return bytes(out), members, 0


def gz(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    """one member by zlib; flush_at: (offset, Z_SYNC_FLUSH or Z_FULL_FLUSH) in ascending order"""
    z = zlib.compressobj(level, zlib.DEFLATED, 31, mem, strategy)
    out, at = b"", 0
    for o, how in flush_at:
        out += z.compress(data[at:o]) + z.flush(how)
        at = o
    return out + z.compress(data[at:]) + z.flush()


def member(raw, data, extra=None, name=None, comment=None, hcrc=False, cm=8, flg_or=0, crc=None, isize=None, bad_hcrc=False):
    """a member around the raw DEFLATE stream `raw` that inflates to `data`, its header written by hand"""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0) | flg_or
    h = bytes([0x1F, 0x8B, cm, flg, 0, 0, 0, 0, 0, 255])
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", (zlib.crc32(h) & 0xFFFF) ^ (1 if bad_hcrc else 0))
    return h + raw + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) & 0xFFFFFFFF if isize is None else isize)


def body_of(m):
    """the raw DEFLATE stream of a member without optional header fields"""
    assert m[3] == 0
    return m[10:-8]


# a complete literal/length set over 14 letters, the end of block and the two lengths 3 and 258, and the distance sets the handmade blocks use
LETTERS = list(b"abcdefghijklmn")
LL = [0] * 286
for _s in LETTERS + [256]:
    LL[_s] = 4
LL[257] = LL[285] = 5
D_FAR = [0] * 29 + [1]                     # distance symbol 29 alone (24577..32768): the one-code set
D_NEAR_FAR = [1] + [0] * 28 + [1]          # distances 1 and 24577..32768


def _letters(n, k=0):
    return [LETTERS[(i * 5 + k) % 14] for i in range(n)]


def distance_32768():
    """32768 stored bytes, then -- at a block start the next chunk finds -- matches of 258 and of 3 bytes at distance exactly 32768"""
    a = np.random.default_rng(11).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    tail = _letters(40)
    w = ic.stored_block(a)
    ic.dynamic_block([(258, 32768), (3, 32768)] + tail, LL, D_FAR, final=False, w=w)
    ic.fixed_block(_letters(9, 3), final=True, w=w)
    data = a + a[:261] + bytes(tail) + bytes(_letters(9, 3))
    return member(w.bytes(), data), data


def ring_hazard():
    """32768 stored bytes; then one batch of tokens: a match of 258 at distance 32768 (it reads the oldest 258 symbols of the ring), five runs of
    258 that carry the batch's output past 1536 symbols, literals -- which a decoder that wrote a batch's literals first and did not cap the
    batch's span would put on the very slots the first match has yet to read -- and at once another match at the maximal distance"""
    a = np.random.default_rng(12).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    toks = [(258, 32768)] + [(258, 1)] * 5 + _letters(300) + [(258, 32768)] + _letters(20, 2)
    w = ic.stored_block(a)
    ic.dynamic_block(toks, LL, D_NEAR_FAR, final=False, w=w)
    ic.fixed_block(_letters(5, 1), final=True, w=w)
    data = bytearray(a)
    for t in toks + _letters(5, 1):
        if isinstance(t, tuple):
            for _ in range(t[0]):
                data.append(data[-t[1]])
        else:
            data.append(t)
    return member(w.bytes(), bytes(data)), bytes(data)


def run_of_one_byte(blocks=12, per=200):
    """non-final dynamic blocks of nothing but matches of 258 at distance 1: every block (and so every chunk) goes on from the byte in front of it"""
    ll = [0] * 286
    ll[97], ll[256], ll[285] = 1, 2, 2
    w = ic.BitWriter()
    for b in range(blocks):
        ic.dynamic_block(([97] if b == 0 else []) + [(258, 1)] * per, ll, [1], final=False, w=w)
    ic.fixed_block([97], final=True, w=w)
    data = b"a" * (2 + 258 * per * blocks)
    return member(w.bytes(), data), data


def motif_text(reps=14, gap=20000):
    """a motif once, then carried forward by matches some 20 KB apart: between two copies text of 16 letters without repeats, which compresses
    to dynamic blocks with no long match of its own"""
    rng = np.random.default_rng(13)
    motif = bytes(rng.integers(128, 256, 64, dtype=np.uint8))
    out = bytearray()
    for _ in range(reps):
        out += motif + bytes(rng.integers(65, 81, gap, dtype=np.uint8))
    return bytes(out + motif), motif


def fixed_tail_bits(extra_bits):
    """a final fixed block whose last bit lies `extra_bits` (1 or -1) behind the 512th bit of the body: 9-bit and 8-bit literals to measure"""
    nine, eight = (7, 55) if extra_bits == 1 else (5, 57)
    toks = [200 + i for i in range(nine)] + [65 + i % 26 for i in range(eight)]
    w = ic.fixed_block(toks, final=True)
    assert w.n == 512 + extra_bits
    return member(w.bytes(), bytes(toks)), bytes(toks)


_CACHE = {}


def cases():
    """name -> Case.  Built once per process"""
    if "all" in _CACHE:
        return _CACHE["all"]
    c = {}
    text = ic.fastq_text(300000, 21)
    small = ic.fastq_text(120000, 22)
    good = lambda data, chunk, slab, expand=16: Case(data, chunk, slab, expand, True, FB_NONE, ARX_OK)
    # 1. levels and many chunks
    for level in (1, 6, 9):
        c["level%d_chunk4096" % level] = good(gz(text, level), 4096, 65536)
        c["level%d_chunk65536" % level] = good(gz(text, level), 65536, 131072)
    c["memlevel1_chunk4096"] = good(gz(small, 6, 1), 4096, 65536)
    c["memlevel1_chunk65536"] = good(gz(small, 6, 1), 65536, 131072)
    c["chunk_below_the_block_spacing"] = good(gz(text, 6), 1024, 131072)
    # 2. markers
    c["distance_32768"] = good(distance_32768()[0], 16384, 65536)
    c["motif_through_many_windows"] = good(gz(motif_text()[0], 9, 5), 8192, 262144)
    c["marker_across_a_launch"] = good(gz(small, 6, 1), 4096, 8192)
    # 3. the ring
    c["ring_hazard"] = good(ring_hazard()[0], 65536, 131072)
    c["run_of_one_byte"] = good(run_of_one_byte()[0], 64, 4096, 1032)
    # 4. block types
    c["level0_stored_only"] = good(gz(small, 0), 4096, 262144)
    c["z_fixed"] = good(gz(small[:60000], 6, 8, zlib.Z_FIXED), 4096, 65536)
    c["flushes"] = good(gz(text[:200000], 6, 8, flush_at=[(777, zlib.Z_SYNC_FLUSH), (30000, zlib.Z_FULL_FLUSH), (30001, zlib.Z_SYNC_FLUSH), (90000, zlib.Z_SYNC_FLUSH),
                                                         (150000, zlib.Z_FULL_FLUSH)]), 4096, 65536)
    for name, (payload, data) in ic.handmade_streams().items():
        c["handmade_" + name] = good(member(payload, data), 64, 4096)
    # 5. framing
    a, b = gz(text[:160000], 6), gz(text[160000:240000], 6)
    c["header_fields"] = good(member(body_of(a), text[:160000], extra=b"XY" + struct.pack("<H", 3) + b"abc", name=b"reads_R1.fastq", comment=b"lane 1", hcrc=True), 4096, 262144)
    c["two_members"] = good(a + b, 4096, 262144)
    parts = [text[:160000], text[160000:240000], text[240000:280000], text[280000:295000], text[295000:]]
    c["five_members"] = good(b"".join(gz(p, 6) for p in parts), 4096, 262144)
    c["two_members_small_slabs"] = good(gz(small, 6, 1) + gz(small[::-1], 6, 1), 2048, 8192)
    empty = gz(b"")
    c["empty_member_first"] = good(empty + a + b, 4096, 262144)
    c["empty_member_in_the_middle"] = good(a + empty + a, 4096, 262144)
    c["empty_member_last"] = good(a + b + empty, 4096, 262144)
    on = member(ic.stored_block(small[:123], final=True).bytes(), small[:123])            # the body is 128 bytes: it ends on the second chunk boundary
    c["member_end_on_a_chunk_boundary"] = good(on + on, 64, 4096)
    c["member_end_a_bit_behind_a_chunk_boundary"] = good(fixed_tail_bits(1)[0] * 2, 64, 4096)
    c["member_end_a_bit_before_a_chunk_boundary"] = good(fixed_tail_bits(-1)[0] * 2, 64, 4096)
    c["trailing_zeros"] = good(a + b"\0" * 100, 4096, 262144)
    c["trailing_bytes"] = good(a + b"no gzip header here, \x1f\x8b or not", 4096, 262144)
    c["lone_1f_at_the_end"] = good(a + b"\x1f", 4096, 262144)
    # 6. slabs
    w = ic.stored_block(small[:121])                                                        # the second block's LEN lies across the 128th byte
    ic.stored_block(small[121:200], final=True, w=w)
    c["slab_end_inside_a_stored_len"] = good(member(w.bytes(), small[:200]), 64, 128)
    c["slab_end_inside_a_trailer"] = good(member(ic.stored_block(small[:119], final=True).bytes(), small[:119]) + on, 64, 128)
    c["block_larger_than_a_slab"] = Case(gz(text, 6), 4096, 8192, 16, False, FB_NO_BLOCK, ARX_OK)
    # 7. forced fallbacks: the right bytes all the same
    c["gzip_inside_stored_blocks"] = Case(gz(gz(text, 6), 0), 4096, 262144, 16, False, FB_REFUTED, ARX_OK)
    c["overflow"] = Case(gz(b"A" * 1000000, 6), 64, 4096, 8, False, FB_OVERFLOW, ARX_OK)
    c["thirty_tiny_members"] = Case(b"".join(gz(b"@r%d\nACGT\n+\nIIII\n" % i) for i in range(30)), 64, 1024, 16, False, FB_CUT_SHORT, ARX_OK)
    # 8. damage: an error, and nothing else
    bad = lambda data, chunk=4096, slab=65536: Case(data, chunk, slab, 16, False, None, ARX_E_IO)
    whole = gz(text, 6)
    flipped = bytearray(whole)
    flipped[len(whole) * 6 // 10] ^= 0x10
    c["damage_flipped_bit_in_a_late_chunk"] = bad(bytes(flipped))
    ra, rb = body_of(a), body_of(b)
    da, db = text[:160000], text[160000:240000]
    c["damage_crc_first_member"] = bad(member(ra, da, crc=zlib.crc32(da) ^ 1) + b, 4096, 262144)
    c["damage_crc_last_member"] = bad(a + member(rb, db, crc=zlib.crc32(db) ^ 0x80000000), 4096, 262144)
    c["damage_isize_first_member"] = bad(member(ra, da, isize=len(da) + 1) + b, 4096, 262144)
    c["damage_isize_last_member"] = bad(a + member(rb, db, isize=len(db) - 1), 4096, 262144)
    c["damage_truncated_in_a_block"] = bad(whole[:len(whole) // 2])
    c["damage_truncated_in_a_trailer"] = bad(whole[:-3])
    c["damage_truncated_in_a_header"] = bad(a + b[:5], 4096, 262144)
    c["damage_cm_7"] = bad(member(ra, da, cm=7) + b, 4096, 262144)
    c["damage_reserved_flag_on_the_second_member"] = bad(a + member(rb, db, flg_or=0x20), 4096, 262144)
    c["damage_fhcrc"] = bad(member(ra, da, name=b"x", hcrc=True, bad_hcrc=True), 4096, 262144)
    _CACHE["all"] = c
    return c


def deflate_blocks(m):
    """the DEFLATE blocks (inflatecases.scan's dicts) of a member without optional header fields"""
    return ic.scan(body_of(m))[1]


# ---- running a case through the host twin, and what every run of a case must give
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ("members", "compressed_bytes", "inflated_bytes", "launches", "chunks", "candidates", "accepted", "refuted", "deflate_blocks", "markers", "host_bytes", "fallback",
         "ignored_bytes")
STABLE = ("members", "chunks", "candidates", "accepted", "refuted", "deflate_blocks", "fallback")     # what does not depend on scheduling


def build_sim(folder, sanitize=True):
    """the host twin (tests/gunzipsim/gunzip_sim.cpp) -> its path.  sanitize: under AddressSanitizer and UBSan, which is the CPU test's build; the
    GPU test wants the twin's counts only and builds it plain"""
    exe = os.path.join(folder, "gunzip_sim")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall"] + san + [os.path.join(ROOT, "tests", "gunzipsim", "gunzip_sim.cpp"), "-o", exe, "-lz"])
    return exe


def run_sim(sim, tmp, case, rev=False):
    """-> dict(rc, out, and the statistics by name)"""
    src, dst = os.path.join(tmp, "in.gz"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(case.data)
    r = subprocess.run([sim, src, dst, str(case.chunk), str(case.slab), str(case.expand)] + (["rev"] if rev else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]               # 3: the reader and gzread disagree
    v = [int(x) for x in r.stdout.split()]
    with open(dst, "rb") as fh:
        res = dict(rc=ARX_OK if v[0] == 0 else ARX_E_IO, out=fh.read())
    res.update(zip(STATS, v[1:]))
    return res


def check(case, res, name):
    """what every run of a case must give, whoever ran it"""
    want = expected(case.data)
    assert res["rc"] == case.ret == (ARX_OK if want is not None else ARX_E_IO), name
    if want is None:
        assert res["out"] == b"", name
        return
    data, members, ignored = want
    assert res["out"] == data, name
    assert res["members"] == members and res["inflated_bytes"] == len(data) and res["ignored_bytes"] == ignored, name
    assert res["compressed_bytes"] == len(case.data) - ignored, name
    assert res["accepted"] <= res["candidates"] <= res["chunks"] and res["host_bytes"] <= len(data), name
    assert (res["fallback"] == 0) == (res["host_bytes"] == 0) or res["fallback"] == FB_CUT_SHORT, name
    assert res["refuted"] == 0 or res["fallback"] != 0, name
    if case.clean:
        assert res["host_bytes"] == 0 and res["fallback"] == 0, (name, res["fallback"])
        assert res["launches"] >= max(members, 1 if data else 0) and res["accepted"] >= res["launches"], name
    elif case.reason is not None:
        assert res["fallback"] == case.reason and res["host_bytes"] > 0, (name, res["fallback"])

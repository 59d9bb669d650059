"""Inputs and the independent reader of the device BGZF tests (test_bgzf_sim.py, test_bgzf_device_gpu.py): every decoded byte is checked by
Python's zlib, zlib.crc32 and struct, never by code under test."""
import struct
import zlib

import numpy as np

BLOCK_IN = 65280
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_blocks(raw):
    """-> [(inflated bytes, bytes of the whole block)]; checks magic, XLEN = 6, the BC subfield of length 2, BSIZE, CRC-32 and ISIZE"""
    out, o = [], 0
    while o < len(raw):
        assert raw[o:o + 4] == b"\x1f\x8b\x08\x04", o
        assert struct.unpack_from("<H", raw, o + 10)[0] == 6 and raw[o + 12:o + 14] == b"BC" and struct.unpack_from("<H", raw, o + 14)[0] == 2, o
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        assert bsize <= 65536 and o + bsize <= len(raw)
        crc, isize = struct.unpack_from("<II", raw, o + bsize - 8)
        data = zlib.decompress(raw[o + 18:o + bsize - 8], -15)   # raises on an invalid code set, a distance too far back, a missing end
        assert len(data) == isize and zlib.crc32(data) == crc and isize <= BLOCK_IN
        out.append((data, bsize))
        o += bsize
    return out


def check_stream(raw, data):
    """raw: framed blocks without the EOF block; they must inflate to data, cut at multiples of 65280 -> the blocks' sizes"""
    blocks = bgzf_blocks(raw)
    assert [b for b, _ in blocks] == [data[o:o + BLOCK_IN] for o in range(0, len(data), BLOCK_IN)]
    return [s for _, s in blocks]


def _text(rng, n):
    words = [b"the", b"quick", b"brown", b"fox", b"jumps", b"over", b"lazy", b"dog", b"BX:Z:", b"ACGT", b"\0\0\0", b"arachne"]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(len(words)))] + bytes([int(rng.integers(32, 40))])
    return bytes(out[:n])


def fibonacci(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def edge_inputs():
    """the inputs (a) to (h): name -> bytes; the same seeded bytes on every call"""
    rng = np.random.default_rng(20)
    cases = {}
    for n in (1, 2, 3, 4, 257, 258, 259, 260, 65279, 65280, 65281, 130561):
        cases["a_text_%d" % n] = _text(rng, n)
    cases["b_zeros"] = b"\0" * BLOCK_IN
    cases["b_ff"] = b"\xff" * BLOCK_IN
    rec = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    cases["c_record300"] = (rec * (BLOCK_IN // 300 + 1))[:BLOCK_IN]
    a = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    cases["d_distance_32768"] = a + a[:32512]
    cases["e_distance_32769"] = a + b"\x5a" + a[:32511]
    cases["f_random"] = rng.integers(0, 256, 2 * BLOCK_IN + 1000, dtype=np.uint8).tobytes()
    cases["g_one_value"] = b"a" * 70000
    cases["g_two_values"] = b"ab" * 35000
    v = np.concatenate([np.full(f, 65 + i, np.uint8) for i, f in enumerate(fibonacci(22))])
    assert len(v) == 46367
    rng.shuffle(v)
    cases["h_fibonacci"] = v.tobytes()
    return cases


def check_case(name, data, raw, forms=None):
    """what holds for case `name` beyond inflating to the input; forms: dict(blocks, stored, fixed, dynamic) or None"""
    sizes = check_stream(raw, data)
    if name.startswith("b_"):
        assert len(raw) <= 1024, len(raw)          # distance 1, the longest matches: 253 matches x 13 bits = 638 bytes with the fixed code
    if name == "f_random":
        assert all(s <= min(BLOCK_IN, len(data) - k * BLOCK_IN) + 31 for k, s in enumerate(sizes))
        if forms is not None:
            assert forms["stored"] == forms["blocks"] == len(sizes)
    if forms is not None:
        assert forms["blocks"] == len(sizes) == forms["stored"] + forms["fixed"] + forms["dynamic"]


def bam_like_stream(n, seed=7):
    """n BAM records as the path writes them for 2 x 150 bp reads: barcoded names, one CIGAR operation, 150 packed bases, qualities binned
    to four levels (probabilities .02 / .05 / .13 / .8), the e2e tag set -> the uncompressed record stream"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    levels = np.array([2, 12, 23, 37], np.uint8)
    code4 = np.array([1, 2, 4, 8], np.uint8)
    bc = ""
    for i in range(n):
        if i % 40 == 0:
            bc = "".join("ACGT"[k] for k in rng.integers(0, 4, 18))
        name = ("A00519:%d:H7:%d:%d:%d:%d" % (100 + i // 20000, 1 + (i // 5000) % 4, 1101 + (i // 50) % 80, int(rng.integers(1000, 30000)),
                                              int(rng.integers(1000, 30000)))).encode() + b"\0"
        code = code4[rng.integers(0, 4, 150)]
        packed = (code[0::2] << 4 | code[1::2]).astype(np.uint8).tobytes()
        qual = levels[rng.choice(4, 150, p=[.02, .05, .13, .8])].tobytes()
        aux = b"RGZlib1\0ASC" + bytes([int(rng.integers(100, 151))]) + b"XMZ0\0AMZ1\0XTC\0BXZ" + bc.encode() + b"-1\0VXC\x01"
        pos = int(rng.integers(0, 200_000_000))
        core = struct.pack("<iiBBHHHiiii", 0, pos, len(name), 60, 4681 + (pos >> 14), 1, 99 if i % 2 == 0 else 147, 150, 0, pos + 200, 350)
        body = core + name + struct.pack("<I", 150 << 4) + packed + qual + aux
        out += struct.pack("<i", len(body)) + body
    return bytes(out)


def zlib_size(data, strategy):
    """bytes of the BGZF file zlib level 1 with `strategy` makes of data's blocks (26 bytes of framing each, no EOF block)"""
    total = 0
    for o in range(0, len(data), BLOCK_IN):
        c = zlib.compressobj(1, zlib.DEFLATED, -15, 8, strategy)
        total += len(c.compress(data[o:o + BLOCK_IN]) + c.flush()) + 26
    return total

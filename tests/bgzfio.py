"""A small BGZF writer and splitter for the tests of the device inflate (inflatecases.py, test_feeder_bgzf.py) and for tools/feeder_bench.py.
Everything here is Python's zlib and struct: independent of the code under test.

A BGZF file is a chain of gzip members of at most 65536 bytes, each with an extra subfield BC that holds the member's size minus one, a raw
DEFLATE stream, the CRC-32 and the size of its inflated bytes (the SAM specification, 4.1)."""
import struct
import zlib

BLOCK_IN = 65280            # what samtools and htslib cut at
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def frame(payload, crc, isize, extra_front=b"", cm=8, flg=4):
    """one block around a raw DEFLATE stream; extra_front: whole subfields placed in front of BC"""
    xlen = len(extra_front) + 6
    bsize = 12 + xlen + len(payload) + 8 - 1
    assert bsize < 65536, bsize
    return (struct.pack("<BBBBIBBH", 0x1f, 0x8b, cm, flg, 0, 0, 0xff, xlen) + extra_front + b"BC" + struct.pack("<HH", 2, bsize) + payload +
            struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF))


def deflate_raw(data, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(data) + c.flush()


def block(data, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, extra_front=b""):
    return frame(deflate_raw(data, level, mem_level, strategy), zlib.crc32(data), len(data), extra_front)


def cut_points(n, cut):
    """cut: a block size, or the ascending offsets at which a new block starts -> [(from, to)] that tile [0, n)"""
    if isinstance(cut, int):
        return [(o, min(n, o + cut)) for o in range(0, n, cut)]
    edges = [0] + [int(c) for c in cut] + [n]
    assert edges == sorted(edges)
    return list(zip(edges[:-1], edges[1:]))


def write_bgzf(data, cut=BLOCK_IN, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, eof=True):
    """data as a BGZF chain, cut every `cut` bytes or at the offsets given (two equal offsets give an empty block); eof: the EOF block behind"""
    out = [block(data[a:b], level, mem_level, strategy) for a, b in cut_points(len(data), cut)]
    if eof:
        out.append(EOF_BLOCK)
    return b"".join(out)


def write_bgzf_file(path, data, **kw):
    raw = write_bgzf(data, **kw)
    with open(path, "wb") as f:
        f.write(raw)
    return raw


def split(raw):
    """a chain -> [dict(at, size, payload, crc, isize)], walking the extra subfields for BC"""
    out, o = [], 0
    while o < len(raw):
        assert raw[o:o + 2] == b"\x1f\x8b" and raw[o + 3] & 4, o
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        p, bsize = o + 12, None
        while p + 4 <= o + 12 + xlen:
            slen = struct.unpack_from("<H", raw, p + 2)[0]
            if raw[p:p + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", raw, p + 4)[0] + 1
                break
            p += 4 + slen
        assert bsize is not None and o + bsize <= len(raw), o
        crc, isize = struct.unpack_from("<II", raw, o + bsize - 8)
        out.append(dict(at=o, size=bsize, payload=raw[o + 12 + xlen:o + bsize - 8], crc=crc, isize=isize))
        o += bsize
    return out


def inflate(raw):
    """a valid chain -> its bytes, by zlib, every block's CRC-32 and ISIZE checked"""
    out = []
    for b in split(raw):
        data = zlib.decompress(b["payload"], -15)
        assert len(data) == b["isize"] and zlib.crc32(data) == b["crc"]
        out.append(data)
    return b"".join(out)

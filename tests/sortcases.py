"""Shared by tests/test_bam_sort_sim.py (the host program over arachne_amd/csrc/dev_bamsort.h) and tests/test_bam_sort_gpu.py (the product's
kernels through arx_selftest_bam_sort): BAM record streams built here with struct, each with what the coordinate sort must make of it, taken
from Python's stable `sorted` over the key ((uint32_t)refID, pos).  Nothing here comes from the code under test.

cases() -> {name: Case}; broken() -> {name: bytes} (chains that must be refused); check_cases() asserts from the bytes that every case is
what its name claims, at every segment size the tests run (SEGS)."""
import functools
import struct

import numpy as np

import reccases

SEGS = (64, 256, 4096)      # the seg_bytes of the tests: a border of the largest is a border of all
N_REF = 3
PROBE_DEPTH = 4             # dev_bamsort.h: BS_PROBE_DEPTH -- the records a guess must chain through
COPY_ALIGN = 8              # dev_bamsort.h: bs_copy moves words of that many bytes at the destination's alignment


def rec(rid, pos, name, l_seq=0, aux=b"", flag=0, mapq=0, mrid=-1, mpos=-1, tlen=0, cigar=()):
    """one BAM record, block_size and all; bases and qualities are a function of l_seq"""
    name = name if isinstance(name, bytes) else name.encode()
    body = struct.pack("<iiBBHHHiiii", rid, pos, len(name) + 1, mapq, 4680, len(cigar), flag, l_seq, mrid, mpos, tlen) + name + b"\0"
    body += b"".join(struct.pack("<I", c) for c in cigar) + bytes((17 * k + 1) & 0xff for k in range((l_seq + 1) // 2)) + bytes(k % 41 for k in range(l_seq)) + aux
    return struct.pack("<i", len(body)) + body


def filler(size, rid=0, pos=5, tag=b"f"):
    """a record of exactly `size` bytes (>= 38)"""
    assert size >= 38
    if size <= 36 + 255:
        return rec(rid, pos, tag * (size - 37))
    r = rec(rid, pos, tag, aux=b"coZ" + b"x" * (size - 38 - 4) + b"\0")
    assert len(r) == size
    return r


def key(r):
    rid, pos = struct.unpack_from("<ii", r, 4)
    return (rid & 0xFFFFFFFF, pos)


class Case:
    def __init__(self, recs, n_ref=N_REF):
        self.recs, self.n_ref = list(recs), n_ref
        self.stream = b"".join(self.recs)
        self.sorted = sorted(self.recs, key=key)                       # stable
        self.out = b"".join(self.sorted)
        self.rec_off = np.concatenate([[0], np.cumsum([len(r) for r in self.sorted], dtype=np.int64)]).astype(np.int64)
        self.in_off = np.concatenate([[0], np.cumsum([len(r) for r in self.recs], dtype=np.int64)]).astype(np.int64)
        self.n = len(self.recs)


def _mixed(rng, n, name=lambda i: b"m%d" % i, l_seq=lambda i: 0):
    return [rec(int(rng.integers(-1, N_REF)), int(rng.integers(-1, 50)), name(i), l_seq=l_seq(i)) for i in range(n)]


def _decoy():
    """a host record whose B:C array holds 6 well-formed fake records back to back: the array's first byte is the first byte of a 4096-byte
    segment, its last byte the host record's last"""
    fakes = b"".join(rec(1, 7 + k, b"fake%d" % k, l_seq=30 + k, mrid=1, mpos=9) for k in range(6))
    name = b"host"
    head = 36 + len(name) + 1 + 8                                           # the host record up to the array's first byte
    front = [rec(0, 100 + k, b"a%d" % k, l_seq=50) for k in range(20)]
    at = sum(len(r) for r in front)
    front.append(filler(4096 - head - at))                                 # so that the host record starts at 4096 - head
    host = rec(2, 3, name, aux=b"dyBC" + struct.pack("<I", len(fakes)) + fakes)
    return front + [host] + [rec(0, 1 + k, b"z%d" % k, l_seq=20) for k in range(30)]


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20250905)
    c = {}
    c["empty"] = Case([])
    c["one_minimal"] = Case([rec(1, 4, b"q")])
    front = [rec(0, 9 - k, b"b%d" % k, l_seq=11 * k) for k in range(9)]
    front.append(filler(4096 - sum(len(r) for r in front), rid=1))
    c["start_on_border"] = Case(front + [rec(0, 2, b"onborder", l_seq=40), rec(-1, -1, b"u"), rec(0, 1, b"last")])
    c["spans_segments"] = Case([rec(1, 5, b"s0"), rec(0, 8, b"long", l_seq=11500), rec(0, 3, b"s1", l_seq=10), rec(-1, -1, b"s2")])
    body = [rec(int(rng.integers(0, N_REF)), int(rng.integers(0, 9)), b"e%d" % k, l_seq=int(rng.integers(0, 90))) for k in range(40)]
    at = sum(len(r) for r in body)
    c["ends_on_last_byte"] = Case(body + [filler(2 * 4096 - at, rid=0, pos=0)])
    c["all_keys_equal"] = Case([rec(1, 77, b"k%d" % k, l_seq=k % 60) for k in range(300)])
    asc = [rec(k // 100, k % 100, b"o%d" % k, l_seq=k % 7) for k in range(300)]
    c["sorted_input"] = Case(asc)
    c["reversed_input"] = Case(asc[::-1])
    c["unmapped_scattered"] = Case([rec(-1, -1, b"u%d" % k, l_seq=k % 33) if k % 3 == 1 else rec(k % N_REF, (k * 7) % 40, b"m%d" % k, l_seq=k % 50) for k in range(400)])
    c["ties"] = Case([rec(1, 1000, b"t%04d" % k) for k in range(1500)] + [rec(0, 5, b"x"), rec(2, 0, b"y")] + [rec(1, 1000, b"t%04d" % k) for k in range(1500, 3000)] +
                     [rec(1, 999, b"w")])
    lens = np.concatenate([rng.permutation(254) + 1 for _ in range(8)])       # every length from 1 to 254, in random order
    c["name_lengths"] = Case([rec(int(rng.integers(-1, N_REF)), int(rng.integers(-1, 30)), bytes(65 + (k + j) % 26 for j in range(int(l)))) for k, l in enumerate(lens)])
    c["seventy_thousand"] = Case(_mixed(rng, 70000, name=lambda i: bytes([97 + i % 26])))
    c["decoy"] = Case(_decoy())
    return c


@functools.lru_cache(maxsize=None)
def broken():
    good = [rec(0, k, b"g%d" % k, l_seq=k) for k in range(12)]
    s = b"".join(good)
    at = sum(len(r) for r in good[:5])
    return {
        "block_size_10": s[:at] + struct.pack("<i", 10) + s[at + 4:],
        "last_record_past_the_end": s[:-5],
        "shorter_than_36": rec(0, 1, b"short")[:20],
    }


def looks_like_record(s, o, n_ref):
    """the probe's test of one offset (the issue's list), restated -> the offset behind the record, or None"""
    if o + 36 > len(s):
        return None
    bs, rid, pos, l_name, _mq, _bin, n_cig, _fl, l_seq, mrid, mpos, _tl = struct.unpack_from("<iiiBBHHHiiii", s, o)
    if bs < 32 or not (-1 <= rid < n_ref and -1 <= mrid < n_ref) or pos < -1 or mpos < -1 or l_seq < 0 or l_name < 2:
        return None
    if 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs or o + 4 + bs > len(s) or s[o + 36 + l_name - 1] != 0:
        return None
    return o + 4 + bs


def chains(s, o, n_ref, depth):
    for d in range(depth):
        if o == len(s) and d > 0:
            return True
        o = looks_like_record(s, o, n_ref)
        if o is None:
            return False
    return True


def check_cases():
    c = cases()
    S = SEGS[-1]
    assert all(S % g == 0 for g in SEGS)
    for name, case in c.items():
        off, _ = reccases.walk(case.stream) if case.n else (np.zeros(1, np.int64), [])
        assert off.tolist() == case.in_off.tolist() and len(case.out) == len(case.stream), name          # the chain tiles the stream
        assert sorted(case.recs) == sorted(case.sorted), name
        ks = [key(r) for r in case.sorted]
        assert ks == sorted(ks), name
    assert c["empty"].stream == b"" and len(c["one_minimal"].stream) == 38
    assert S in c["start_on_border"].in_off.tolist()[1:-1]
    span = c["spans_segments"]
    assert max(np.diff(span.in_off)) > 3 * S + S and any(b // S - a // S > 3 for a, b in zip(span.in_off[:-1], span.in_off[1:]))
    assert len(c["ends_on_last_byte"].stream) % S == 0
    assert len({key(r) for r in c["all_keys_equal"].recs}) == 1 and c["all_keys_equal"].out == c["all_keys_equal"].stream
    assert c["sorted_input"].out == c["sorted_input"].stream and c["reversed_input"].out != c["reversed_input"].stream
    assert sorted(map(key, c["reversed_input"].recs), reverse=True) == list(map(key, c["reversed_input"].recs))
    um = c["unmapped_scattered"]
    un = [r for r in um.recs if key(r)[0] == 0xFFFFFFFF]
    assert 100 < len(un) < um.n and um.sorted[-len(un):] == un and key(um.recs[0])[0] != 0xFFFFFFFF and key(um.recs[-1])[0] != 0xFFFFFFFF
    ties = [r for r in c["ties"].sorted if key(r) == (1, 1000)]
    assert len(ties) == 3000 and [r[36:41] for r in ties] == [b"t%04d" % k for k in range(3000)] and c["ties"].out != c["ties"].stream
    nl = c["name_lengths"]
    assert {r[12] - 1 for r in nl.recs} >= set(range(1, 255))
    src = {id(r): o for r, o in zip(nl.recs, nl.in_off)}
    assert len({(src[id(r)] % COPY_ALIGN, int(o) % COPY_ALIGN) for r, o in zip(nl.sorted, nl.rec_off)}) == COPY_ALIGN * COPY_ALIGN
    assert c["seventy_thousand"].n == 70000 > 65535 and len(c["seventy_thousand"].stream) == 70000 * 38
    d = c["decoy"]
    host = [k for k, r in enumerate(d.recs) if r[36:40] == b"host"][0]
    a, b = int(d.in_off[host]), int(d.in_off[host + 1])
    assert a < S < b and S not in d.in_off.tolist()                                       # the border lies inside the host record ...
    assert d.stream[S - 8:S - 4] == b"dyBC" and chains(d.stream, S, d.n_ref, PROBE_DEPTH + 2)     # ... at the array's first byte, where fake records chain
    o = S
    for _ in range(6):
        o = looks_like_record(d.stream, o, d.n_ref)
    assert o == b                                                                         # and end with the host record
    for name, s in broken().items():
        try:
            reccases.walk(s)
        except (AssertionError, struct.error, ValueError):
            continue
        raise AssertionError(name + " walks")
    assert len(broken()["shorter_than_36"]) < 36

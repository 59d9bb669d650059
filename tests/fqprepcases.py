"""Shared by tests/test_fastq_prepare_sim.py (the host program over arachne_amd/csrc/dev_fqprep.h) and tests/test_fastq_prepare_gpu.py (the product's
kernels through arx_selftest_fastq_prepare and arx_fastq_prepare): raw FASTQ text pairs, each with what the fused call must make of it.  The
expectation is the two existing restatements composed -- fqsortcases.Case over the texts that fqstdcases.Case makes of the input, or over the
input itself where the detection finds the standard form --, which is the rule of the call: the bytes of arx_fastq_sort_ex after
arx_fastq_standardize.  Nothing here comes from the code under test.

cases() -> {name: Case}; check_cases() asserts from the bytes that every case is what its name claims."""
import functools

import numpy as np

import fqsortcases as fc
import fqstdcases as sc

AUTO, HAPLOTAGGING, STLFR, TELLSEQ, STANDARD, UNKNOWN = range(6)
WINDOWS, SLABS = fc.WINDOWS, fc.SLABS
RUN_BYTES = (128, 256, 4096)
COPY_ALIGN = fc.COPY_ALIGN
GATHER_LANES = 16           # dev_fqsort.h: FS_GATHER_LANES


def key_rule(ident, bc):
    """the sort key by the rule of include/arachne_amd.h (arx_fastq_prepare), stated on id and barcode"""
    return ident.split(b"BX:Z:", 1)[1] + b"/1" if b"BX:Z:" in ident else bc


class Case:
    """std: fqstdcases' view of the input (format, found, decided, used, fields ...); exp: fqsortcases' view of what is sorted -- None where
    AUTO finds no format.  found / decided: what the call reports as the format and the record that decided it (forced: the format, -1)"""

    def __init__(self, t1, t2, fmt=AUTO, claims=()):
        self.t1, self.t2, self.format, self.claims = bytes(t1), bytes(t2), fmt, tuple(claims)
        self.std = s = sc.Case(t1, t2, fmt, claims)
        self.found, self.decided = (s.found, s.decided) if fmt == AUTO else (fmt, -1)
        self.windows = s.windows
        self.run_bytes = sc.WIDE_WINDOWS if "wide" in self.claims else RUN_BYTES
        self.skipped = s.skipped
        self.with_bc = self.valid = 0
        if s.used is not None:
            self.exp = fc.Case(s.out1, s.out2)
            self.with_bc, self.valid = s.with_bc, s.valid
            assert self.exp.skipped == 0 and self.exp.n == s.n
        elif s.found == STANDARD:
            self.exp = fc.Case(t1, t2)
        else:
            self.exp = None
        if self.exp is not None:
            e = self.exp
            self.n, self.out1, self.out2, self.off1, self.off2 = e.n, e.out1, e.out2, e.off1, e.off2
            self.runs, self.distinct, self.longest = e.runs, e.distinct, e.longest


rec = sc.rec
_text = sc._text


def _key_in_id():
    """the id holds BX:Z: -- the issue's examples, a tie between a key in two pieces and a real barcode of the same bytes, an id that is only the tag"""
    hs = [b"q BX:Z:zz", b"xBX:Z:ab BX:Z:cd", b"y BX:Z:ab/1", b"zBX:Z:ab/1", b"p BX:Z:ab", b"BX:Z:A01C02B03D04", b"r BX:Z:A01C02B03D04", b"wBX:Z: BX:Z:m", b"y2 BX:Z:ab/1",
          b"s BX:Z:ab/0", b"t BX:Z:ab/2", b"uBX:Z:BX:Z:k"]
    return _text([rec(h, 4 + k % 5, 3 + k % 4, k) for k, h in enumerate(hs)])


_S = b"KLMNOPQRSTUVWXYZ"
TWO_PIECE_LENGTHS = (7, 8, 9, 15, 16, 17)


def _key_edges():
    """keys in two pieces of lengths 7 .. 17: the "/1" before, across and behind the edge of an 8-byte chunk, each between two real barcodes that
    differ from it only in the last byte"""
    hs = []
    for n in TWO_PIECE_LENGTHS:
        s = _S[:n - 2]
        hs += [b"a%d BX:Z:%s/2" % (n, s), b"b%dBX:Z:%s BX:Z:other" % (n, s), b"c%d BX:Z:%s/0" % (n, s), b"d%d BX:Z:%s/" % (n, s), b"e%d BX:Z:%s/1x" % (n, s)]
    return _text([rec(h, 3 + k % 6, 2 + k % 5, k) for k, h in enumerate(hs)])


def _key_stlfr():
    hs = [b"a#5_5_6/1", b"bBX:Z:5_5_5#1_2_3/1", b"c#5_5_4/1", b"d#5_5_5/1", b"eBX:Z:#9_9_9", b"f#1_2_3/1", b"BX:Z:5_5_5#7_7_7/2"]
    return _text([rec(h, 4 + k % 5, 3 + k % 4, k) for k, h in enumerate(hs)])


def _key_tell():
    hs = [b"a:TTTT", b"tBX:Z:AC:ACGT", b"c:AC", b"d:AD x:AC", b"BX:Z:AC:G", b"e:ACGT"]
    return _text([rec(h, 4 + k % 5, 3 + k % 4, k) for k, h in enumerate(hs)])


HEADER_LENGTHS = (17, 18, 31, 32, 33, 34)


def _header_lengths():
    """composed headers of 17 (empty id and barcode) .. 34 bytes against the 16 gather lanes, every length with three barcodes in falling order"""
    hs = []
    for n in HEADER_LENGTHS:
        extra = n - 17
        for bc in (b"T", b"G", b"A"):
            if extra == 0:
                hs.append(b"")
            elif extra == 1:
                hs.append(b"i")
            else:
                nb = extra // 2
                hs.append((b"j" * (extra - nb)) + b" :" + bc * nb)
    return _text([rec(h, 2 + k % 7, 1 + k % 6, k) for k, h in enumerate(hs)])


def _alignment(n=448, seed=17):
    """id, barcode and read lengths vary so that lines 2-4 meet every (source, destination) alignment of the copy in both files"""
    rng = np.random.default_rng(seed)
    pool = [b"ACGT"[k % 4:k % 4 + 1] * (1 + k % 9) for k in range(36)]
    ps = []
    for k in range(n):
        ident = (b"%d" % k + b"n" * 8)[:1 + (k * 3) % 8]
        l1 = 1 + k % 37
        l2 = 1 + (l1 + 5 + k % 4) % 37
        ps.append(rec(ident + b" :" + pool[int(rng.integers(len(pool)))], l1, l2, k))
    return _text(ps)


def _run_borders():
    """about 9 kB a file: barcodes in rows of three, a skipped line every fourth record, keys in two pieces in the last third"""
    t1, t2 = [], []
    for k in range(160):
        g = (k // 3 * 7) % 11
        h = b"r%d#%d_2_3/1" % (k, g) if k < 120 or k % 5 else b"r%dBX:Z:%d#4_5_6/1" % (k, g)
        a, b = rec(h, 8 + k % 9, 6 + k % 7, k)
        t1.append(a)
        t2.append(b)
        if k % 4 == 3:
            t1.append(b"stray line %d\n" % k)
            t2.append(b"s\n")
    return b"".join(t1), b"".join(t2)


def _standard():
    ps = [fc.pair(b"o%d" % k, bc, 5, 4, k, extra=b"\tVX:i:%d" % (k % 2)) for k, bc in enumerate([b"T-1", b"A-9", b"T-1", b"C-4", b"A-9", b"A"])]
    return _text(ps)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    for name in sc.cases():                                               # every case of the standardization at its own format
        s = sc.cases()[name]
        c["std_" + name] = Case(s.t1, s.t2, s.format, s.claims)
    for name in fc.cases():                                               # every case of the sort, read as haplotagging
        s = fc.cases()[name]
        c["sort_" + name] = Case(s.t1, s.t2, HAPLOTAGGING, s.claims)
    c["key_in_id"] = Case(*_key_in_id(), fmt=HAPLOTAGGING, claims=("windows",))
    c["key_edges"] = Case(*_key_edges(), fmt=HAPLOTAGGING, claims=("windows", "chunks"))
    c["key_stlfr"] = Case(*_key_stlfr(), fmt=STLFR)
    c["key_tell"] = Case(*_key_tell(), fmt=TELLSEQ)
    c["header_lengths"] = Case(*_header_lengths(), fmt=TELLSEQ, claims=("windows",))
    c["alignment"] = Case(*_alignment(), fmt=TELLSEQ, claims=("windows", "slabs", "align"))
    c["run_borders"] = Case(*_run_borders(), claims=("windows", "runs", "skipped"))
    c["standard_auto"] = Case(*_standard())
    return c


LARGE = ("std_many", "sort_many")
SMALL = tuple(n for n in cases() if n not in LARGE)
UNKNOWN_CASES = tuple(n for n in SMALL if cases()[n].exp is None)
GOOD = tuple(n for n in SMALL if cases()[n].exp is not None)


def check_cases():
    cs = cases()
    assert {"std_" + n for n in sc.SMALL} | {"sort_" + n for n in fc.SMALL} <= set(SMALL)
    for name, c in cs.items():
        s = c.std
        if s.used is None:
            continue
        # the key of every record is the rule's, and the expectation orders by it, stably
        keys = [key_rule(f[0], f[1]) for f in s.fields]
        assert keys == [r[2] for r in c.exp.recs], name
        order = sorted(range(c.n), key=lambda k: keys[k])
        assert c.out1 == b"".join(s.parts1[k] for k in order) and c.out2 == b"".join(s.parts2[k] for k in order), name
    assert sum(1 for n in cs if n.startswith("std_") and cs[n].std.used is not None and cs[n].out1 != cs[n].std.out1) >= 11   # they come out in another order
    c = cs["std_three_hundred"]
    assert (c.runs, c.distinct) == (75, 73)
    for n in fc.SMALL:                                                    # read as haplotagging the sort's cases keep their keys
        assert [r[2] for r in cs["sort_" + n].exp.recs] == [r[2] for r in fc.cases()[n].recs], n
    assert {len(r[2]) for r in cs["sort_lengths"].exp.recs} >= set(fc.LENGTHS)
    assert cs["std_det_199"].found == STLFR and cs["std_det_200"].exp is None and cs["std_empty"].exp is None and cs["std_empty_forced"].n == 0
    c = cs["key_in_id"]
    k = [r[2] for r in c.exp.recs]
    assert k[1] == k[2] == k[3] == k[8] == b"ab/1" and k[5] == b"A01C02B03D04/1" and k[6] == b"A01C02B03D04" and k[7] == b"/1" and k[11] == b"BX:Z:k/1"
    assert c.std.fields[1] == (b"xBX:Z:ab", b"ab", 1) and c.std.fields[3] == (b"zBX:Z:ab", b"ab/1", 1) and c.std.fields[5][0] == b"BX:Z:A01C02B03D04"
    tie = [r[0].split(b"/1\t")[0] for r in c.exp.sorted if r[2] == b"ab/1"]
    assert tie == [b"@xBX:Z:ab", b"@y", b"@zBX:Z:ab", b"@y2"]                # input order among the equal keys, whichever form they have
    assert c.runs == len(k) - 2 and c.distinct == len(set(k)) == len(k) - 3  # ... and they count as one key
    c = cs["key_edges"]
    k = [r[2] for r in c.exp.recs]
    assert {len(x) for x, f in zip(k, c.std.fields) if b"BX:Z:" in f[0]} == set(TWO_PIECE_LENGTHS)
    for n in TWO_PIECE_LENGTHS:
        s = _S[:n - 2]
        got = [x for x in (r[2] for r in c.exp.sorted) if x.startswith(s + b"/") and len(x) <= n + 1]
        assert got == [s + b"/", s + b"/0", s + b"/1", s + b"/1x", s + b"/2"], (n, got)
    c = cs["key_stlfr"]
    assert [r[2] for r in c.exp.sorted] == [b"#9_9_9/1", b"1_2_3", b"5_5_4", b"5_5_5", b"5_5_5#1_2_3/1", b"5_5_5#7_7_7/1", b"5_5_6"]
    c = cs["key_tell"]
    assert [r[2] for r in c.exp.sorted] == [b"AC", b"AC", b"AC:ACGT/1", b"AC:G/1", b"ACGT", b"TTTT"]
    c = cs["header_lengths"]
    for parts in (c.std.parts1, c.std.parts2):
        assert sorted({len(p.split(b"\n", 1)[0]) + 1 for p in parts}) == list(HEADER_LENGTHS)
    assert c.std.fields[0][:2] == (b"", b"") and c.out1 != c.std.out1
    c = cs["alignment"]
    order = sorted(range(c.n), key=lambda k: c.exp.recs[k][2])
    for raw, parts, out_off in (([r[0] for r in c.std.recs], c.std.parts1, c.off1), ([r[1] for r in c.std.recs], c.std.parts2, c.off2)):
        in_off = fc._offsets(raw)
        seen = set()
        for j, k in enumerate(order):
            src = int(in_off[k]) + len(raw[k].split(b"\n", 1)[0]) + 1        # where lines 2-4 start in the input
            dst = int(out_off[j]) + len(parts[k].split(b"\n", 1)[0]) + 1     # ... and in the output
            seen.add((src % COPY_ALIGN, dst % COPY_ALIGN))
        assert len(seen) == COPY_ALIGN * COPY_ALIGN, len(seen)
    c = cs["run_borders"]
    assert c.found == STLFR and c.skipped == 40 and len(c.t1) > 4096 + 1024 and len(c.t2) > 4096
    two = [k for k, f in enumerate(c.std.fields) if b"BX:Z:" in f[0]]
    assert two and int(fc._offsets([r[0] for r in c.std.recs])[two[0]]) > 4096   # a key in two pieces lies behind the first run of every size
    assert c.runs > c.distinct and max(len(r[0]) for r in c.std.recs) < 128
    c = cs["standard_auto"]
    assert c.found == STANDARD and c.std.used is None and c.out1 != c.t1 and sorted(c.out1.split(b"\n")) == sorted(c.t1.split(b"\n")) and c.runs > c.distinct

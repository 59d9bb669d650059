"""Shared by tests/test_fastq_sort_sim.py (the host program over arachne_amd/csrc/dev_fqsort.h) and tests/test_fastq_sort_gpu.py (the product's
kernels through arx_selftest_fastq_sort and arx_fastq_sort): FASTQ text pairs built here from bytes, each with what the sort by barcode must
make of it.  The expectation is a restatement of the contract (include/arachne_amd.h: arx_fastq_sort) in Python over `bytes`: lines exist
only where they end in a newline, the two files' lines are walked in lockstep, a line pair whose R1 line starts with '@' opens a record of
four line pairs when the walk is searching, other lines are skipped, a record the end of either file cuts off does not exist; the barcode
is the leftmost BX:Z:(\\S+)\\s of the R1 header with its newline; the order is Python's stable sorted() over the barcodes, which compares
bytes unsigned and puts a proper prefix first.  Nothing here comes from the code under test.

cases() -> {name: Case}; check_cases() asserts from the bytes that every case is what its name claims."""
import functools
import re

import numpy as np

MIN_WINDOW = 128            # dev_fqsort.h: FS_MIN_WINDOW -- every line and every record of the cases fits it
WINDOWS = (MIN_WINDOW, 256, 4096)
SLABS = (1, 4096)           # slab_bytes: one record a slab, and a few dozen
COPY_ALIGN = 8              # dev_bamsort.h: bs_copy moves words of that many bytes at the destination's alignment
BX = re.compile(rb"BX:Z:(\S+)\s")


def barcode(header_line):
    """header_line: the R1 header without its newline"""
    m = BX.search(header_line + b"\n")
    return m.group(1) if m else b""


def records(t1, t2):
    """-> ([(r1 bytes, r2 bytes, barcode)] in input order, lines skipped)"""
    l1, l2 = t1.split(b"\n")[:-1], t2.split(b"\n")[:-1]
    n = min(len(l1), len(l2))
    recs, skipped, j = [], 0, 0
    while j < n:
        if l1[j][:1] != b"@":
            skipped += 1
            j += 1
            continue
        if j + 4 > n:
            break                                        # cut off by the end of a file: it does not exist
        recs.append((b"".join(x + b"\n" for x in l1[j:j + 4]), b"".join(x + b"\n" for x in l2[j:j + 4]), barcode(l1[j])))
        j += 4
    return recs, skipped


def _offsets(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts], dtype=np.int64)]).astype(np.int64)


class Case:
    def __init__(self, t1, t2, claims=()):
        self.t1, self.t2, self.claims = bytes(t1), bytes(t2), tuple(claims)
        self.recs, self.skipped = records(self.t1, self.t2)
        self.sorted = sorted(self.recs, key=lambda r: r[2])                # stable; bytes compare unsigned, a proper prefix first
        self.n = len(self.recs)
        self.out1, self.out2 = b"".join(r[0] for r in self.sorted), b"".join(r[1] for r in self.sorted)
        self.off1, self.off2 = _offsets([r[0] for r in self.sorted]), _offsets([r[1] for r in self.sorted])
        self.in_off1, self.in_off2 = _offsets([r[0] for r in self.recs]), _offsets([r[1] for r in self.recs])
        bcs = [r[2] for r in self.recs]
        self.runs = sum(1 for k, b in enumerate(bcs) if k == 0 or b != bcs[k - 1])
        self.distinct = len(set(bcs))
        self.longest = max([len(b) for b in bcs], default=0)


_SEQ = b"ACGTTGCAAGCTNACGGATCCATGACTGATCGATCGGCTAAGCTTACG"
_QUAL = bytes(range(35, 35 + 29)) * 2                # '#' .. '?': never '@'


def pair(name, bc, l1=5, l2=4, k=0, extra=b"", plus1=b"+", q1=None):
    """one record: the R1 header is @name[ BX:Z:bc][extra]; R2's header carries no barcode.  k moves the windows the bases are cut from"""
    h = b"@" + name + (b"" if bc is None else b" BX:Z:" + bc) + extra
    a, b = k % 7, (3 * k) % 5
    q = _QUAL[a:a + l1] if q1 is None else q1
    r1 = h + b"\n" + _SEQ[a:a + l1] + b"\n" + plus1 + b"\n" + q + b"\n"
    r2 = b"@" + name + b"/2\n" + _SEQ[b:b + l2] + b"\n+\n" + _QUAL[b:b + l2] + b"\n"
    return r1, r2


def _text(pairs):
    return b"".join(p[0] for p in pairs), b"".join(p[1] for p in pairs)


_LONG = b"ACGTACGTTGCATGCAACGTACGTT"                  # 25 bytes: its prefixes are the barcodes of the lengths under test
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 25)


def _lengths():
    bcs = [None if n == 0 else _LONG[:n] for n in LENGTHS]
    bcs += [b"AB", b"AB\x00", b"AB\x00\x00", b"\x80A", b"zA", b"A\xff", b"A\x7f",
            _LONG[:15] + b"A", _LONG[:15] + b"C",        # 16 bytes, differ in the last byte of the last chunk
            _LONG[:7] + b"\x01", _LONG[:7] + b"\x02",    # 8 bytes, the same
            _LONG[:23] + b"\xfe", _LONG[:23] + b"\xff"]  # 24 bytes, the same
    order = list(reversed(range(len(bcs)))) + list(range(0, len(bcs), 2)) + list(range(1, len(bcs), 3))
    return _text([pair(b"l%d" % i, bcs[o], 3 + i % 4, 2 + i % 3, i) for i, o in enumerate(order)])


def _header_forms():
    ps = [pair(b"h0", b"zz"),
          pair(b"h1", None, extra=b" BX:Z: BX:Z:x"),                 # BX:Z: followed by a space is no match; the real one follows
          pair(b"h2", None, extra=b" VX:i:1 BX:Z:"),                 # BX:Z: as the last token: no barcode
          pair(b"h3", b"x", extra=b"\tVX:i:1"),
          pair(b"h4", None, extra=b"\tVX:i:0\tBX:Z:y"),              # the value is closed by the header's own newline
          pair(b"h5", b"y", extra=b" BX:Z:other"),                   # the leftmost match counts
          pair(b"h6", None, extra=b" xBX:Z:q\r"),                    # the match may start anywhere; '\r' closes the value
          pair(b"h7", None)]
    return _text(ps)


def _stability():
    runs = [(b"B-1", 3), (b"A-1", 2), (b"B-1", 2), (b"C-1", 1), (b"B-1", 3)]
    ps, k = [], 0
    for bc, n in runs:
        for _ in range(n):
            ps.append(pair(b"s%d" % k, bc, 4 + k % 3, 3 + k % 2, k))
            k += 1
    return _text(ps)


def _sorted_clean():
    bcs = [None, None, b"A", b"A", b"AA", b"AB", b"AB", b"B-1", b"B-10", b"\xc3\xa9"]
    return _text([pair(b"o%d" % k, bc, 5, 6, k) for k, bc in enumerate(bcs)])


def _reverse():
    bcs = [b"T-9", b"T-1", b"G-2", b"G-2", b"C", b"A-1", None]
    return _text([pair(b"v%d" % k, bc, 6, 5, k) for k, bc in enumerate(bcs)])


def _alignment(n=640, seed=11):
    """read lengths 1..40, R2's differ from R1's, name lengths vary, the barcodes come in a seeded order"""
    rng = np.random.default_rng(seed)
    pool = [b"A-%d" % k for k in range(23)] + [_LONG[:9 + k] for k in range(8)]
    ps = []
    for k in range(n):
        l1 = 1 + k % 40
        l2 = 1 + (l1 + 6 + k % 3) % 40
        assert l1 != l2
        ps.append(pair(b"a" * (k % 5) + b"%d" % k, pool[int(rng.integers(len(pool)))], l1, l2, k))
    return _text(ps)


def _bad_lines():
    r = [pair(b"b%d" % k, bc, 5, 4, k) for k, bc in enumerate([b"Q", b"P", b"Q", b"P", b"O"])]
    r[1] = pair(b"b1", b"P", 5, 4, 1, q1=b"@#$%&")                    # a quality line that starts with '@': inside a record it is no header
    r[2] = pair(b"b2", b"Q", 5, 4, 2, plus1=b"+b2 again")             # a '+' line with text
    bad = (b"stray\n", b"other stray\n")
    t1 = bad[0] + b"\n" + r[0][0] + r[1][0] + b"not a header\n+\n" + r[2][0] + r[3][0] + b"ACGT\n" + r[4][0] + b"trailing\n\n"
    t2 = bad[1] + b"x\n" + r[0][1] + r[1][1] + b"@looks like one\nz\n" + r[2][1] + r[3][1] + b"\n" + r[4][1] + b"t\nu\n"
    return t1, t2


def _r2_short():
    ps = [pair(b"t%d" % k, bc, 4, 4, k) for k, bc in enumerate([b"B", b"A", b"B", b"A"])]
    t1, t2 = _text(ps)
    return t1, t2[:-len(ps[-1][1])] + b"".join(x + b"\n" for x in ps[-1][1].split(b"\n")[:2])   # the last record's R2 has two lines


def _no_final_newline():
    t1, t2 = _text([pair(b"n%d" % k, bc, 4, 4, k) for k, bc in enumerate([b"B", b"A", b"0"])])
    return t1[:-1], t2


def _three_lines():
    ps = [pair(b"e%d" % k, bc, 4, 4, k) for k, bc in enumerate([b"B", b"A", b"0"])]
    t1, t2 = _text(ps)
    cut = lambda t, r: t[:-len(r)] + b"".join(x + b"\n" for x in r.split(b"\n")[:3])
    return cut(t1, ps[-1][0]), cut(t2, ps[-1][1])


def _three_hundred(seed=5):
    rng = np.random.default_rng(seed)
    pool = [b"ACGTACGTAC-%d" % k for k in range(40)]
    return _text([pair(b"m%d" % k, pool[int(rng.integers(len(pool)))], 20 + k % 9, 18 + k % 11, k) for k in range(300)])


def _many(n=70000, seed=9):
    """tiny records, about 3 MB a file: the radix sort leaves its single-block path"""
    rng = np.random.default_rng(seed)
    pool = [b"%s-%d" % (_LONG[k % 7:k % 7 + 8 + k % 6], k) for k in range(5000)]
    pick = rng.integers(len(pool), size=n)
    r1 = [b"@r%d BX:Z:%s\nACGT\n+\n#$%%&\n" % (k, pool[int(pick[k])]) for k in range(n)]
    r2 = [b"@r%d/2\nTTGCA\n+\n#$%%&'\n" % k for k in range(n)]
    return b"".join(r1), b"".join(r2)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["lengths"] = Case(*_lengths(), claims=("windows", "chunks"))
    c["header_forms"] = Case(*_header_forms(), claims=("windows",))
    c["stability"] = Case(*_stability(), claims=("windows",))
    c["one_barcode"] = Case(*_text([pair(b"u%d" % k, b"SAME-1", 5, 5, k) for k in range(10)]), claims=("windows",))
    c["sorted_clean"] = Case(*_sorted_clean(), claims=("windows",))
    c["reverse"] = Case(*_reverse(), claims=("windows",))
    c["alignment"] = Case(*_alignment(), claims=("windows", "blocks", "slabs", "align"))
    c["bad_lines"] = Case(*_bad_lines(), claims=("windows", "skipped"))
    c["r2_short"] = Case(*_r2_short())
    c["no_final_newline"] = Case(*_no_final_newline())
    c["three_lines"] = Case(*_three_lines())
    c["empty"] = Case(b"", b"")
    c["empty_r2"] = Case(pair(b"x", b"A")[0], b"")
    c["one"] = Case(*pair(b"only", b"A-1", 7, 9))
    c["three_hundred"] = Case(*_three_hundred(), claims=("windows", "blocks", "slabs"))
    c["many"] = Case(*_many(), claims=("windows", "blocks", "slabs", "large"))
    return c


SMALL = tuple(n for n in ("lengths", "header_forms", "stability", "one_barcode", "sorted_clean", "reverse", "alignment", "bad_lines", "r2_short", "no_final_newline",
                          "three_lines", "empty", "empty_r2", "one", "three_hundred"))


def check_cases():
    cs = cases()
    assert set(SMALL) | {"many"} == set(cs)
    for name, c in cs.items():
        for t in (c.t1, c.t2):                                            # every line and every record fits the smallest window
            assert max([len(x) + 1 for x in t.split(b"\n")], default=0) <= MIN_WINDOW, name
        assert all(len(r[0]) <= MIN_WINDOW and len(r[1]) <= MIN_WINDOW for r in c.recs), name
        assert [r[2] for r in c.sorted] == sorted(r[2] for r in c.recs), name
    c = cs["lengths"]
    bcs = [r[2] for r in c.recs]
    assert {len(b) for b in bcs} >= set(LENGTHS) and c.longest == 25
    assert b"AB" in bcs and b"AB\x00" in bcs and any(b[0] >= 0x80 for b in bcs if b)
    srt = [r[2] for r in c.sorted]
    assert srt.index(b"AB") < srt.index(b"AB\x00") < srt.index(b"AB\x00\x00")                 # a proper prefix first, NUL or not
    assert srt.index(b"zA") < srt.index(b"\x80A") and srt.index(b"A\x7f") < srt.index(b"A\xff")   # unsigned bytes
    assert srt.index(_LONG[:7]) < srt.index(_LONG[:8]) < srt.index(_LONG[:9])
    for a, b in ((_LONG[:15] + b"A", _LONG[:15] + b"C"), (_LONG[:7] + b"\x01", _LONG[:7] + b"\x02"), (_LONG[:23] + b"\xfe", _LONG[:23] + b"\xff")):
        assert len(a) % 8 == 0 and a[:-1] == b[:-1] and srt.index(a) < srt.index(b)
    assert srt[0] == b"" and c.runs > c.distinct
    c = cs["header_forms"]
    assert [r[2] for r in c.recs] == [b"zz", b"x", b"", b"x", b"y", b"y", b"q", b""]
    c = cs["stability"]
    b_names = [r[0].split(b" ")[0] for r in c.sorted if r[2] == b"B-1"]
    assert len(b_names) == 8 and b_names == [r[0].split(b" ")[0] for r in c.recs if r[2] == b"B-1"] and c.runs == 5 and c.distinct == 3
    assert len({r[0] for r in c.recs}) == c.n and len({r[1] for r in c.recs}) == c.n                # every record distinguishable
    c = cs["one_barcode"]
    assert c.runs == c.distinct == 1 and c.out1 == c.t1 and c.out2 == c.t2
    c = cs["sorted_clean"]
    assert c.skipped == 0 and c.out1 == c.t1 and c.out2 == c.t2 and c.runs == c.distinct < c.n
    c = cs["reverse"]
    assert c.sorted == [c.recs[k] for k in (6, 5, 4, 2, 3, 1, 0)] and c.runs == c.distinct == 6
    c = cs["alignment"]
    l1 = {len(r[0].split(b"\n")[1]) for r in c.recs}
    assert l1 == set(range(1, 41)) and all(len(r[0].split(b"\n")[1]) != len(r[1].split(b"\n")[1]) for r in c.recs)
    by_key = {id(r): k for k, r in enumerate(c.recs)}
    for in_off, out_off, which in ((c.in_off1, c.off1, 0), (c.in_off2, c.off2, 1)):
        seen = {(int(in_off[by_key[id(r)]]) % COPY_ALIGN, int(out_off[j]) % COPY_ALIGN) for j, r in enumerate(c.sorted)}
        assert len(seen) == COPY_ALIGN * COPY_ALIGN, (which, len(seen))                          # all 8 x 8 (source, destination) alignments
    c = cs["bad_lines"]
    assert c.n == 5 and c.skipped == 7 and c.t1.startswith(b"stray") and c.t1.endswith(b"trailing\n\n")
    assert any(r[0].split(b"\n")[3][:1] == b"@" for r in c.recs) and any(len(r[0].split(b"\n")[2]) > 1 for r in c.recs)
    c = cs["r2_short"]
    assert c.n == 3 and c.t2.count(b"\n") == c.t1.count(b"\n") - 2 and c.skipped == 0
    c = cs["no_final_newline"]
    assert c.n == 2 and not c.t1.endswith(b"\n")
    c = cs["three_lines"]
    assert c.n == 2 and c.t1.count(b"\n") == 11
    assert cs["empty"].n == 0 and cs["empty_r2"].n == 0 and cs["one"].n == 1
    c = cs["three_hundred"]
    assert c.n == 300 and c.skipped == 0 and c.runs > c.distinct > 1
    c = cs["many"]
    assert c.n == 70000 and 2_500_000 < len(c.t1) < 3_500_000 and c.distinct > 4000

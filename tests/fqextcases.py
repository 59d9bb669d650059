"""Shared by tests/test_fastq_sort_ext_sim.py (the host program over arachne_amd/csrc/dev_fqmerge.h) and tests/test_fastq_sort_ext_gpu.py (the
product's kernels through arx_selftest_fastq_sort_ext and arx_fastq_sort_ex): FASTQ text pairs whose point is the border between two sorted
runs of the external sort.  The expectation is fqsortcases' restatement of the contract (Case.out1, .out2, .off1, .off2, .runs, .distinct,
.skipped, .longest): what the sort makes of an input does not depend on run_bytes.  Every case carries the run_bytes it is meant for and the
least number of sorted runs it must produce there: a run holds at most run_bytes of either file, so an output of B bytes in a file needs
ceil(B / run_bytes) runs at least.  check_cases() verifies both from the bytes alone, so that no case passes through a single run by accident.

cases() -> {name: ExtCase}; an ExtCase with status != 0 is refused at its run_bytes (and says nothing about other sizes)."""
import functools

import fqsortcases as fc

RUN_BYTES = (fc.MIN_WINDOW, 256, 4096)       # the smallest allowed at the smallest window, and two more
MAX_RUNS = 1024                              # dev_fqmerge.h: FS_MAX_RUNS
FS_E_RUN, FS_E_RUNS = 3, 4                   # dev_fqmerge.h: a run cannot hold a record; too many runs
GATHER_LANES = 16                            # dev_fqsort.h: FS_GATHER_LANES


def least_runs(case, run_bytes):
    return max(-(-len(case.out1) // run_bytes), -(-len(case.out2) // run_bytes))


class ExtCase:
    def __init__(self, t1, t2, run_bytes=fc.MIN_WINDOW, status=0, exact_runs=None):
        self.case = fc.Case(t1, t2)
        self.run_bytes, self.status, self.exact_runs = run_bytes, status, exact_runs
        self.min_runs = least_runs(self.case, run_bytes)


def _text(pairs):
    return b"".join(p[0] for p in pairs), b"".join(p[1] for p in pairs)


def _spread(n=40):
    """every second record carries the one barcode; the names number them"""
    return _text([fc.pair(b"s%02d" % k, b"SAME" if k % 2 == 0 else b"o%d" % (9 - k % 7), 5, 4, k) for k in range(n)])


def _long_r1(n=30):
    """R1's records are about nine times R2's: the files' run borders fall in different records, R2's carry spans several"""
    return _text([fc.pair(b"%d" % (k % 10), b"L%d" % ((7 * k) % 5), 40, 1, k) for k in range(n)])


def _pad_to(lines1, target, rb):
    """lines1: R1's lines, the first being a skipped line that may grow: -> the lines, with line `target` ending at byte rb exactly"""
    pad = 0
    for extra in range(0, 100):
        ls = list(lines1)
        ls[pad] = ls[pad] + b"j" * extra
        end = sum(len(l) + 1 for l in ls[:target + 1])
        if end == rb:
            return ls
    raise AssertionError("no padding puts line %d's end at %d" % (target, rb))


def _skips_at_border(shift, rb=fc.MIN_WINDOW):
    """a skipped line, two records, a skipped line, a three-line fragment, more records.  The second skipped line ends `shift` lines before (-1), exactly at (0) or
    after (1) the first run's end -- byte rb of R1, the first run's buffer starting at the file's start"""
    head = [fc.pair(b"k%d" % k, b"Z%d" % (3 - k), 5, 4, k) for k in range(2)]
    tail = [fc.pair(b"t%d" % k, b"Y%d" % ((5 * k) % 4), 5, 4, k) for k in range(8)]
    l1 = [b"pad"] + b"".join(p[0] for p in head).split(b"\n")[:-1] + [b"junk"] + [b"@frag BX:Z:F", b"ACG", b"+"] + b"".join(p[0] for p in tail).split(b"\n")[:-1]
    l2 = [b"p"] + b"".join(p[1] for p in head).split(b"\n")[:-1] + [b"x"] + [b"@frag/2", b"TTT", b"+"] + b"".join(p[1] for p in tail).split(b"\n")[:-1]
    l1 = _pad_to(l1, 9 - shift, rb)               # line 9 is the skipped one
    return b"".join(l + b"\n" for l in l1), b"".join(l + b"\n" for l in l2)


def _late(end):
    ps = [fc.pair(b"e%02d" % k, b"B%d" % ((3 * k) % 5), 5, 4, k) for k in range(14)]
    t1, t2 = _text(ps)
    lines = lambda r, n: b"".join(x + b"\n" for x in r.split(b"\n")[:n])
    if end == "cut":                              # the last record has three lines in both files
        return t1[:-len(ps[-1][0])] + lines(ps[-1][0], 3), t2[:-len(ps[-1][1])] + lines(ps[-1][1], 3)
    if end == "r2_short":                         # the last record's R2 has two lines
        return t1, t2[:-len(ps[-1][1])] + lines(ps[-1][1], 2)
    return t1[:-1], t2                            # R1's last line has no newline


def _borders():
    """R1 records of 32 bytes: at run_bytes 128 a run is four records.  B continues over the first border, C ends on the second"""
    bcs = [b"DDDA", b"DDDA", b"DDDB", b"DDDB", b"DDDB", b"DDDB", b"DDDC", b"DDDC", b"AAAA", b"AAAA", b"AAAA", b"AAAA", b"DDDB", b"AAAA"]
    return _text([fc.pair(b"b" + bytes([65 + k]), bc, 7, 3, k) for k, bc in enumerate(bcs)])


_L = fc._LONG
_PARTNERS = ((b"AB", b"AB\x00"), (None, b"\x00"), (_L[:7], _L[:8]), (_L[:8], _L[:9]), (_L[:16], _L[:17]), (_L[:9], _L[:7]), (_L[:17], _L[:16]))


def _prefixes():
    """the first of every pair early, fillers, the second late: the equal-prefix partners lie in different runs"""
    first = [fc.pair(b"p%d" % k, a, 4, 3, k) for k, (a, b) in enumerate(_PARTNERS)]
    fill = [fc.pair(b"f%d" % k, b"M%d" % (k % 3), 4, 3, k) for k in range(6)]
    second = [fc.pair(b"q%d" % k, b, 4, 3, k) for k, (a, b) in enumerate(_PARTNERS)]
    return _text(first + fill + second)


def _sorted(n=60, reverse=False):
    ks = range(n - 1, -1, -1) if reverse else range(n)
    return _text([fc.pair(b"n%02d" % k, b"S%02d" % (k // 2), 5, 4, k) for k in ks])


def _wide(n=80):
    """four barcodes in turn: every output slab of 4096 bytes draws from every run"""
    return _text([fc.pair(b"w%02d" % k, b"W%d" % (k % 4), 5, 4, k) for k in range(n)])


def _too_long():
    t1, t2 = _text([fc.pair(b"r%d" % k, b"A%d" % k, 5, 4, k) for k in range(6)])
    big = fc.pair(b"n" * 150, b"A", 5, 4)
    return big[0] + t1, big[1] + t2


def _over_cap():
    n = 4 * MAX_RUNS + 4                          # R1 records of 32 bytes, four to a run of 128
    return _text([fc.pair(b"%04d" % k, b"C%d" % (k % 7), 7, 3, k) for k in range(n)])


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["spread"] = ExtCase(*_spread())
    c["long_r1"] = ExtCase(*_long_r1())
    for shift in (-1, 0, 1):
        c["skips_%s" % ("before", "at", "after")[shift + 1]] = ExtCase(*_skips_at_border(shift))
    c["cut_late"] = ExtCase(*_late("cut"))
    c["r2_short_late"] = ExtCase(*_late("r2_short"))
    c["no_newline_late"] = ExtCase(*_late("no_newline"))
    c["borders"] = ExtCase(*_borders())
    c["prefixes"] = ExtCase(*_prefixes())
    c["sorted_runs"] = ExtCase(*_sorted())
    c["reverse_runs"] = ExtCase(*_sorted(reverse=True))
    c["wide_slab"] = ExtCase(*_wide())
    c["too_long"] = ExtCase(*_too_long(), status=FS_E_RUN)
    c["over_cap"] = ExtCase(*_over_cap(), status=FS_E_RUNS)
    c["one_run"] = ExtCase(*fc._stability(), run_bytes=4096, exact_runs=1)
    c["zero"] = ExtCase(b"", b"", exact_runs=0)
    c["only_skipped"] = ExtCase(b"a\nb\nc\n" * 60, b"x\ny\n" * 90, exact_runs=0)
    return c


GOOD = tuple(n for n, x in cases().items() if x.status == 0)
REFUSED = tuple(n for n, x in cases().items() if x.status != 0)


def check_cases():
    cs = cases()
    for name, x in cs.items():
        c, rb = x.case, x.run_bytes
        if name != "too_long":
            for t in (c.t1, c.t2):
                assert max([len(l) + 1 for l in t.split(b"\n")], default=0) <= fc.MIN_WINDOW, name
            assert all(len(r[0]) <= fc.MIN_WINDOW and len(r[1]) <= fc.MIN_WINDOW for r in c.recs), name
        assert x.min_runs == least_runs(c, rb)
        if x.exact_runs is None and x.status == 0:
            assert x.min_runs >= 2, name                                    # no case passes through a single run
    bcs = lambda c: [r[2] for r in c.recs]
    x = cs["spread"]
    c = x.case
    assert all(b == b"SAME" for b in bcs(c)[::2]) and b"SAME" not in bcs(c)[1::2]
    assert all(4 * len(r[0]) <= x.run_bytes for r in c.recs)               # a run holds three records at least, so one of the barcode's
    same = [r[0].split(b" ")[0] for r in c.sorted if r[2] == b"SAME"]
    assert same == sorted(same) and len(same) == 20 and x.min_runs >= 8
    x = cs["long_r1"]
    c = x.case
    assert all(len(r[0]) >= 6 * len(r[1]) for r in c.recs) and x.min_runs >= 20
    for shift, nm in ((-1, "skips_before"), (0, "skips_at"), (1, "skips_after")):
        x = cs[nm]
        l1 = x.case.t1.split(b"\n")[:-1]
        ends = [sum(len(l) + 1 for l in l1[:k + 1]) for k in range(len(l1))]
        assert l1[9] == b"junk" and ends[9 - shift] == x.run_bytes, nm
        assert x.case.skipped >= 2 and l1[10].startswith(b"@frag") and x.case.n >= 9, nm
    assert cs["skips_at"].case.skipped == cs["skips_before"].case.skipped == cs["skips_after"].case.skipped
    x = cs["cut_late"]
    assert x.case.n == 13 and x.case.t1.count(b"\n") == 55 and x.min_runs >= 3
    x = cs["r2_short_late"]
    assert x.case.n == 13 and x.case.t2.count(b"\n") == x.case.t1.count(b"\n") - 2 and x.min_runs >= 3
    x = cs["no_newline_late"]
    assert x.case.n == 13 and not x.case.t1.endswith(b"\n") and x.min_runs >= 3
    x = cs["borders"]
    c = x.case
    assert x.run_bytes == 128 and all(len(r[0]) == 32 and len(r[1]) < 32 for r in c.recs)      # so a run is four records
    b = bcs(c)
    assert b[3] == b[4] and b[7] != b[8] and b[6] == b[7] and b[11] != b[12] and c.runs == 6 and c.distinct == 4
    x = cs["prefixes"]
    c = x.case
    starts = dict(zip([r[0].split(b" ")[0].split(b"\n")[0] for r in c.recs], c.in_off1.tolist()))
    for k, (a, bb) in enumerate(_PARTNERS):
        assert starts[b"@q%d" % k] - starts[b"@p%d" % k] >= x.run_bytes                           # no run holds both
    assert {len(v) for v in bcs(c)} >= {0, 1, 2, 3, 7, 8, 9, 16, 17}
    srt = [r[2] for r in c.sorted]
    assert srt.index(b"AB") < srt.index(b"AB\x00") and srt[0] == b"" and srt.index(b"") < srt.index(b"\x00")
    x = cs["sorted_runs"]
    assert x.case.out1 == x.case.t1 and x.case.runs == x.case.distinct == 30 and x.min_runs >= 10
    x = cs["reverse_runs"]
    assert x.case.sorted[0] is x.case.recs[-2] and x.case.runs == x.case.distinct == 30 and x.min_runs >= 10
    x = cs["wide_slab"]
    assert x.min_runs > GATHER_LANES and len(x.case.out1) <= 4096 and len(x.case.out2) <= 4096    # one slab of 4096 bytes, all runs in it
    x = cs["too_long"]
    assert len(x.case.recs[0][0]) > x.run_bytes and len(x.case.t1) > 2 * x.run_bytes
    x = cs["over_cap"]
    assert x.min_runs == MAX_RUNS + 1
    x = cs["one_run"]
    assert len(x.case.t1) <= x.run_bytes and len(x.case.t2) <= x.run_bytes and x.case.n > 1
    assert cs["zero"].case.n == 0 and cs["only_skipped"].case.n == 0 and cs["only_skipped"].case.skipped == 180

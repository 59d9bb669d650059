"""Shared by tests/test_fastq_standardize_sim.py (the host program over arachne_amd/csrc/dev_fqstd.h) and tests/test_fastq_standardize_gpu.py (the
product's kernels through arx_selftest_fastq_standardize and arx_fastq_standardize): FASTQ text pairs built here from bytes, each with what the
header standardization must make of it.  The expectation is a restatement of the contract (include/arachne_amd.h: arx_fastq_standardize) in
Python: `re` over `bytes`, whose \\s is the six bytes of the feeder's white space, and bytes.split(), which splits at the same six.  The records
are the sort's (fqsortcases.records, itself a restatement).  Nothing here comes from the code under test.

cases() -> {name: Case}; check_cases() asserts from the bytes that every case is what its name claims."""
import functools
import re

import numpy as np

import fqsortcases as fc

AUTO, HAPLOTAGGING, STLFR, TELLSEQ, STANDARD, UNKNOWN = range(6)      # the format codes of include/arachne_amd.h
NAMES = ("auto", "haplotagging", "stlfr", "tellseq", "standard", "unknown")
MIN_WINDOW = fc.MIN_WINDOW
WINDOWS, SLABS = fc.WINDOWS, fc.SLABS
WIDE_WINDOWS = (1024, 2048, 4096)                                     # for the cases that claim "wide": a record of theirs fits no smaller window
DETECT_RECORDS = 200

BX = re.compile(rb"BX:Z:(\S+)\s")
VX = re.compile(rb"VX:i:([01])\s")
HAP = re.compile(rb"BX:Z:A\d\dC\d\dB\d\dD\d\d\s")
STL = re.compile(rb"#([0-9]+_[0-9]+_[0-9]+)(/[12])?\s")
TEL = re.compile(rb":([ATCGN]+)\s")
STL_INVALID = re.compile(rb"^0_|_0_|_0$")


def classify(H):
    """H: the R1 header without its '@', with its newline -> the first format in the order of trial that it matches, or None"""
    if BX.search(H) and VX.search(H):
        return STANDARD
    if HAP.search(H):
        return HAPLOTAGGING
    if STL.search(H):
        return STLFR
    if TEL.search(H):
        return TELLSEQ
    return None


def detect(headers):
    """-> (format, the record that decided or -1)"""
    for k, H in enumerate(headers[:DETECT_RECORDS]):
        f = classify(H)
        if f is not None:
            return f, k
    return UNKNOWN, -1


def fields(H, fmt):
    """-> (id, barcode, v)"""
    tok = H.split()
    ident = tok[0] if tok else b""
    if ident.endswith((b"/1", b"/2")):
        ident = ident[:-2]
    m = {HAPLOTAGGING: BX, STLFR: STL, TELLSEQ: TEL}[fmt].search(H)
    if not m:
        return ident, b"", 0
    bc = m.group(1)
    if fmt == HAPLOTAGGING:
        v = b"00" not in bc
    elif fmt == STLFR:
        v = not STL_INVALID.search(bc)
    else:
        v = b"N" not in bc
    return ident, bc, int(v)


class Case:
    """format: what the call is given (AUTO detects).  found / decided: the detection's result on the input; used: the format the conversion
    runs in, or None where nothing is written (AUTO found standard or unknown)"""

    def __init__(self, t1, t2, fmt=AUTO, claims=()):
        self.t1, self.t2, self.format, self.claims = bytes(t1), bytes(t2), fmt, tuple(claims)
        self.recs, self.skipped = fc.records(self.t1, self.t2)
        self.n = len(self.recs)
        self.headers = [r[0].split(b"\n", 1)[0][1:] + b"\n" for r in self.recs]
        self.found, self.decided = detect(self.headers)
        self.used = fmt if fmt != AUTO else self.found if self.found in (HAPLOTAGGING, STLFR, TELLSEQ) else None
        self.windows = WIDE_WINDOWS if "wide" in self.claims else WINDOWS
        if self.used is None:
            return
        self.fields = [fields(H, self.used) for H in self.headers]
        o1, o2 = [], []
        for (r1, r2, _), (ident, bc, v) in zip(self.recs, self.fields):
            for out, r, mate in ((o1, r1, b"1"), (o2, r2, b"2")):
                out.append(b"@" + ident + b"/" + mate + b"\tBX:Z:" + bc + b"\tVX:i:" + (b"1" if v else b"0") + b"\n" + r.split(b"\n", 1)[1])
        assert all(len(a) == 17 + len(f[0]) + len(f[1]) + len(r[0].split(b"\n", 1)[1]) for a, f, r in zip(o1, self.fields, self.recs))
        self.parts1, self.parts2 = o1, o2
        self.out1, self.out2 = b"".join(o1), b"".join(o2)
        self.off1, self.off2 = fc._offsets(o1), fc._offsets(o2)
        self.with_bc = sum(1 for f in self.fields if f[1])
        self.valid = sum(f[2] for f in self.fields)
        self.longest = max([len(f[1]) for f in self.fields], default=0)


def rec(hdr, l1=5, l2=4, k=0, **kw):
    """one record whose R1 header is '@' + hdr"""
    return fc.pair(hdr, None, l1, l2, k, **kw)


def _text(pairs):
    return b"".join(p[0] for p in pairs), b"".join(p[1] for p in pairs)


# ---- one record each, under AUTO: what the detection makes of a header
DETECT_ONE = {
    "det_hap": (b"r BX:Z:A01C02B03D04", HAPLOTAGGING),
    "det_hap_short": (b"r BX:Z:A01C02B03D0 x", UNKNOWN),
    "det_hap_long": (b"r BX:Z:A01C02B03D04x", UNKNOWN),
    "det_hap_lower": (b"r BX:Z:a01c02b03d04", UNKNOWN),
    "det_stlfr_two": (b"r#1_2", UNKNOWN),
    "det_stlfr_gap": (b"r#1__2_3", UNKNOWN),
    "det_stlfr_lead": (b"r#_1_2_3", UNKNOWN),
    "det_stlfr_mate3": (b"r#1_2_3/3", UNKNOWN),
    "det_stlfr_mate1": (b"r#1_2_3/1", STLFR),
    "det_stlfr_eol": (b"r#1_2_3", STLFR),
    "det_tell_lower": (b"r:ACGTn x", UNKNOWN),
    "det_tell_none": (b"r: x", UNKNOWN),
    "det_tell_eol": (b"r:ACGT", TELLSEQ),
    "det_second_start": (b"r#1_2 #11_22_33 :AC:GT ", STLFR),
    "det_tell_second": (b"r:AC:GT x", TELLSEQ),
    "det_vt": (b"r:ACGT\x0bx", TELLSEQ),
    "det_both": (b"r#1_2_3 x:ACGT", STLFR),
    "det_hap_vx": (b"r BX:Z:A01C02B03D04 VX:i:1", STANDARD),
    "det_bx_only": (b"r BX:Z:free VX:i:2", UNKNOWN),
    "det_plain": (b"r 1", UNKNOWN),
}


def _detect_at(k, n_after=3):
    """k records that match nothing, then one that says stLFR, then a few more"""
    ps = [rec(b"n%d" % i, 3 + i % 3, 2 + i % 4, i) for i in range(k)]
    ps += [rec(b"s%d#%d_2_3/1" % (i, i + 1), 4, 4, i) for i in range(1 + n_after)]
    return _text(ps)


def _hap_forms():
    hs = [b"h0 BX:Z:A01C02B03D04", b"h1 BX:Z:A01C02B03D0 x", b"h2 BX:Z:A01C02B03D04x", b"h3\tBX:Z:a01c02b03d04\tRX:Z:q", b"h4 BX:Z:A00C01B01D01", b"h5 BX:Z:A10C01B20D30",
          b"h6 BX:Z: BX:Z:A01C01B01D01\x0bBX:Z:A02C02B02D02", b"h7", b"h8/1 BX:Z:A01C02B03D00", b"h9 BX:Z:A01C02B03D04 VX:i:1", b"h10 xBX:Z:0\r", b"h11 BX:Z:"]
    return _text([rec(h, 4 + k % 5, 3 + k % 4, k) for k, h in enumerate(hs)])


STLFR_VALIDITY = ((b"0_1_2", 0), (b"1_0_2", 0), (b"1_2_0", 0), (b"00_1_2", 1), (b"1_00_2", 1), (b"10_20_30", 1))


def _stlfr_forms():
    hs = [b"v%d#%s/1" % (k, bc) for k, (bc, _) in enumerate(STLFR_VALIDITY)]
    hs += [b"w0#7_8_9", b"w1#1_2 #3_4_5/2 #6_7_8", b"w2#1_2_3/3", b"w3", b"w4#12_34_56/1\tsecond", b"w5 #0_0_0 x", b"w6#1_2_3/1/1"]
    return _text([rec(h, 4 + k % 5, 3 + k % 4, k) for k, h in enumerate(hs)])


def _tell_forms():
    hs = [b"t0:NACGT", b"t1:ACGTN", b"t2:ACGT", b"t3", b"t4:ACGTn :GG", b"t5: :T", b"t6:1:2:ACGTACGTACGTACGTAC 1:N:0", b"t7:ACGT\x0bx:CC", b"t8:acgt", b"t9:N"]
    return _text([rec(h, 4 + k % 5, 3 + k % 4, k) for k, h in enumerate(hs)])


def _ids():
    hs = [b"a/1 :AC", b"b/2 :AC", b"c/3 :AC", b"/1 :AC", b"x", b"", b" lead :AC", b"\t\x0bq/1", b"i:ACGT", b"j/1/2", b"/2", b"k/ :A", b" "]
    return _text([rec(h, 3 + k % 4, 2 + k % 5, k) for k, h in enumerate(hs)])


def _lengths():
    """id lengths 0 .. 16 crossed with body lengths: every alignment of a record's start in the output and of its lines 2-4 in the input"""
    ps, k = [], 0
    for rnd in range(8):
        for n in range(17):
            ident = b"/1" if n == 0 else (b"%d" % k + b"q" * 16)[:n]
            ps.append(rec(ident + b" :" + b"ACGTTGCA"[:1 + (k // 3) % 8], 1 + (3 * k + rnd) % 23, 1 + (5 * k + rnd) % 19, k))
            k += 1
    return _text(ps)


def _bc300():
    bc = (b"ACGTTGCAAGCT" * 25)[:300]
    return _text([rec(b"big0:" + bc, 5, 4, 0), rec(b"big1:" + bc[:299] + b"N extra", 6, 7, 1), rec(b"small:AC", 4, 4, 2)])


def _records():
    """fqsortcases' bad lines with stLFR headers: skipped lines, a quality line that starts with '@', a '+' line with text"""
    r = [rec(b"b%d#%d_5_6/1" % (k, k), 5, 4, k) for k in range(5)]
    r[1] = rec(b"b1#1_5_6/1", 5, 4, 1, q1=b"@#$%&")
    r[2] = rec(b"b2#2_5_6/1", 5, 4, 2, plus1=b"+b2 again")
    t1 = b"stray\n\n" + r[0][0] + r[1][0] + b"not a header\n+\n" + r[2][0] + r[3][0] + b"ACGT\n" + r[4][0] + b"trailing\n\n"
    t2 = b"other stray\nx\n" + r[0][1] + r[1][1] + b"@looks like one\nz\n" + r[2][1] + r[3][1] + b"\n" + r[4][1] + b"t\nu\n"
    return t1, t2


def _r2_short():
    ps = [rec(b"t%d:AC" % k, 4, 4, k) for k in range(4)]
    t1, t2 = _text(ps)
    return t1, t2[:-len(ps[-1][1])] + b"".join(x + b"\n" for x in ps[-1][1].split(b"\n")[:2])   # the last record's R2 has two lines


def _cut_off():
    ps = [rec(b"e%d:AC" % k, 4, 4, k) for k in range(3)]
    t1, t2 = _text(ps)
    return t1[:-len(ps[-1][0])] + b"".join(x + b"\n" for x in ps[-1][0].split(b"\n")[:3]), t2   # the last record's R1 has three lines


def _window_end():
    """R1's first record is exactly the smallest window, the second one ends exactly at the second window's end"""
    def exact(name, total):
        r1, r2 = rec(name, 40, 9, 1)
        pad = total - len(r1)
        return rec(name + b"p" * pad, 40, 9, 1)
    return _text([exact(b"w0#1_2_3/1 ", MIN_WINDOW), exact(b"w1#4_5_6/1 ", MIN_WINDOW), rec(b"w2#7_8_9/1", 5, 5, 2)])


def _many(n=4000, seed=13):
    rng = np.random.default_rng(seed)
    a, b, c = (rng.integers(0, 1537, size=n) for _ in range(3))
    r1 = [b"@V3%05dL1C001R%07d#%d_%d_%d/1\nACGTTGCAAGCTNACGGATC\n+\n#$%%&'()*+,-./0123456\n" % (k % 7, k, a[k], b[k], c[k]) for k in range(n)]
    r2 = [b"@V3%05dL1C001R%07d#%d_%d_%d/2\nTTGCAAGCTNACG\n+\n56789:;<=>?AB\n" % (k % 7, k, a[k], b[k], c[k]) for k in range(n)]
    return b"".join(r1), b"".join(r2)


def raw_pair(fmt, n, seed=3, per_barcode=4, l1=20, l2=18):
    """a pair with headers in the raw form of `fmt`, `per_barcode` records per barcode in a row, every few barcodes an invalid one"""
    rng = np.random.default_rng(seed)
    ps = []
    for k in range(n):
        g = k // per_barcode
        if fmt == HAPLOTAGGING:
            h = b"hp%d BX:Z:A%02dC%02dB%02dD%02d" % (k, g % 96 if g % 5 else 0, 1 + g // 96 % 96, 1 + g % 7, 1 + g % 11)
        elif fmt == STLFR:
            h = b"sl%d#%d_%d_%d/1" % (k, g % 1536 if g % 5 else 0, 1 + g % 13, 1 + g // 1536)
        else:
            letters = b"ACGT" if g % 5 else b"ACGN"
            h = b"ts%d:%s" % (k, bytes(letters[int(x)] for x in rng.integers(0, 4, size=18)) if k % per_barcode == 0 else ps[-1][0].split(b"\n")[0].split(b":")[1])
        ps.append(rec(h, l1, l2, k))
    return _text(ps)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    for name, (h, _) in DETECT_ONE.items():
        c[name] = Case(*rec(h, 6, 5))
    c["det_199"] = Case(*_detect_at(199), claims=("windows", "slabs"))
    c["det_200"] = Case(*_detect_at(200))
    c["hap_vx_forced"] = Case(*rec(DETECT_ONE["det_hap_vx"][0], 6, 5), fmt=HAPLOTAGGING)
    c["empty"] = Case(b"", b"")
    c["empty_forced"] = Case(b"", b"", fmt=STLFR)
    c["empty_r2"] = Case(rec(b"x#1_2_3")[0], b"", fmt=STLFR)
    c["hap_forms"] = Case(*_hap_forms(), fmt=HAPLOTAGGING, claims=("windows",))
    c["hap_auto"] = Case(*_hap_forms())
    c["stlfr_forms"] = Case(*_stlfr_forms(), fmt=STLFR, claims=("windows",))
    c["stlfr_auto"] = Case(*_stlfr_forms())
    c["tell_forms"] = Case(*_tell_forms(), fmt=TELLSEQ, claims=("windows",))
    c["tell_auto"] = Case(*_tell_forms())
    c["ids"] = Case(*_ids(), fmt=TELLSEQ, claims=("windows",))
    c["lengths"] = Case(*_lengths(), claims=("windows", "slabs", "align"))
    c["bc300"] = Case(*_bc300(), claims=("wide",))
    c["records"] = Case(*_records(), claims=("windows", "skipped"))
    c["r2_short"] = Case(*_r2_short())
    c["cut_off"] = Case(*_cut_off())
    c["window_end"] = Case(*_window_end(), claims=("windows",))
    c["three_hundred"] = Case(*raw_pair(STLFR, 300), claims=("windows", "slabs"))
    c["many"] = Case(*_many(), claims=("windows", "slabs"))
    return c


SMALL = tuple(n for n in cases() if n != "many")


def check_cases():
    cs = cases()
    for name, c in cs.items():
        room = c.windows[0]
        for t in (c.t1, c.t2):                                            # every line and every record fits the smallest window the case runs at
            assert max([len(x) + 1 for x in t.split(b"\n")], default=0) <= room, name
        assert all(len(r[0]) <= room and len(r[1]) <= room for r in c.recs), name
        assert all(b"BX:Z:" not in H.split()[0] and b"VX:i:" not in H.split()[0] for H in c.headers if H.split()), name   # the property's condition
    for name, (h, want) in DETECT_ONE.items():
        c = cs[name]
        assert c.n == 1 and c.found == want and c.decided == (0 if want != UNKNOWN else -1), (name, c.found)
    assert DETECT_ONE["det_vt"][0].count(b"\x0b") == 1 and DETECT_ONE["det_second_start"][0].index(b"#1_2 ") < DETECT_ONE["det_second_start"][0].index(b"#11_22_33 ")
    c = cs["det_199"]
    assert c.n > 200 and (c.found, c.decided) == (STLFR, 199) and all(classify(H) is None for H in c.headers[:199])
    c = cs["det_200"]
    assert c.n > 200 and (c.found, c.decided, c.used) == (UNKNOWN, -1, None) and classify(c.headers[200]) == STLFR and all(classify(H) is None for H in c.headers[:200])
    assert cs["det_200"].t1.startswith(cs["det_199"].t1[:cs["det_199"].t1.index(b"@s0")])       # the same input, the deciding record one later
    c = cs["hap_vx_forced"]
    assert c.found == STANDARD and c.used == HAPLOTAGGING and c.fields == [(b"r", b"A01C02B03D04", 1)] and cs["det_hap_vx"].used is None
    assert cs["empty"].found == UNKNOWN and cs["empty"].used is None and cs["empty_forced"].n == 0 and cs["empty_forced"].out1 == b"" and cs["empty_r2"].n == 0
    c = cs["hap_forms"]
    assert [f[1:] for f in c.fields] == [(b"A01C02B03D04", 1), (b"A01C02B03D0", 1), (b"A01C02B03D04x", 1), (b"a01c02b03d04", 1), (b"A00C01B01D01", 0), (b"A10C01B20D30", 1),
                                         (b"A01C01B01D01", 1), (b"", 0), (b"A01C02B03D00", 0), (b"A01C02B03D04", 1), (b"0", 1), (b"", 0)]
    assert c.fields[8][0] == b"h8" and cs["hap_auto"].found == HAPLOTAGGING and cs["hap_auto"].out1 == c.out1
    c = cs["stlfr_forms"]
    assert [f[1:] for f in c.fields[:6]] == [(bc, v) for bc, v in STLFR_VALIDITY]
    assert [f[1:] for f in c.fields[6:]] == [(b"7_8_9", 1), (b"3_4_5", 1), (b"", 0), (b"", 0), (b"12_34_56", 1), (b"0_0_0", 0), (b"", 0)]
    assert c.fields[0][0] == b"v0#0_1_2" and c.fields[12][0] == b"w6#1_2_3/1" and cs["stlfr_auto"].found == STLFR and cs["stlfr_auto"].out2 == c.out2
    c = cs["tell_forms"]
    assert [f[1:] for f in c.fields] == [(b"NACGT", 0), (b"ACGTN", 0), (b"ACGT", 1), (b"", 0), (b"GG", 1), (b"T", 1), (b"ACGTACGTACGTACGTAC", 1), (b"ACGT", 1), (b"", 0), (b"N", 0)]
    assert cs["tell_auto"].found == TELLSEQ and cs["tell_auto"].decided == 0
    c = cs["ids"]
    assert [f[0] for f in c.fields] == [b"a", b"b", b"c/3", b"", b"x", b"", b"lead", b"q", b"i:ACGT", b"j/1", b"", b"k/", b""]
    assert c.headers[5] == b"\n" and c.headers[6][:1] == b" "
    c = cs["lengths"]
    assert c.found == TELLSEQ and {len(f[0]) for f in c.fields} == set(range(17))
    body_at = np.array([int(o) + len(r[0].split(b"\n", 1)[0]) + 1 for o, r in zip(fc._offsets([r[0] for r in c.recs]), c.recs)])
    body2_at = np.array([int(o) + len(r[1].split(b"\n", 1)[0]) + 1 for o, r in zip(fc._offsets([r[1] for r in c.recs]), c.recs)])
    for at in (c.off1[:-1], c.off2[:-1], body_at, body2_at):
        assert {int(x) % 16 for x in at} == set(range(16))
    c = cs["bc300"]
    assert c.longest == 300 and c.fields[0][2] == 1 and c.fields[1][2] == 0 and len(c.fields[1][1]) == 300
    c = cs["records"]
    assert c.n == 5 and c.skipped == 7 and any(r[0].split(b"\n")[3][:1] == b"@" for r in c.recs) and c.found == STLFR and c.valid == 4
    assert cs["r2_short"].n == 3 and cs["cut_off"].n == 2 and cs["cut_off"].t1.count(b"\n") == 11
    c = cs["window_end"]
    assert c.n == 3 and len(c.recs[0][0]) == len(c.recs[1][0]) == MIN_WINDOW and c.with_bc == 3
    c = cs["three_hundred"]
    assert c.n == 300 and 0 < c.valid < c.with_bc == 300
    c = cs["many"]
    assert c.n == 4000 and c.found == STLFR and 0 < c.valid < c.n and len(c.out1) > len(c.t1)

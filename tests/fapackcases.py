"""Shared by tests/test_fasta_pack_sim.py (the host program over arachne_amd/csrc/dev_fapack.h) and tests/test_fasta_pack_gpu.py (the product's
kernels through arx_selftest_fasta_pack and arx_index_build_ex): FASTA texts built here from bytes, each with what the index build must make of
it.  The expectation is a restatement of the rules (include/arachne_amd.h: arx_index_build_ex; the rules are arx_index_build's) as one
byte-serial Python loop, its lrand48 stepped and never jumped.  Nothing here comes from the code under test.

cases() -> {name: Case}; check_cases() asserts from the bytes that every case is what its name claims, and that the cuts of 64-byte windows
fall at every place the window carry has to get right."""
import functools

import numpy as np

WINDOWS = (64, 256, 4096)
BLANKS = b"\n\r \t"
OK, BAD_START, EMPTY = 0, 1, 2                    # what the build makes of a text: packed; a base before the first '>'; no base at all
REFUSALS = {BAD_START: "FASTA does not start with '>'", EMPTY: "empty FASTA"}


def nt4(b):
    """nst_nt4_table: A/C/G/T in either case -> 0..3, '-' -> 5, everything else -> 4"""
    i = b"ACGT".find(bytes([b]).upper()) if bytes([b]).isalpha() else -1
    return i if i >= 0 else 5 if b == 0x2D else 4


class Rand48:
    """srand48(seed); lrand48(): the top 31 bits of X' = (0x5DEECE66D X + 0xB) mod 2^48"""

    def __init__(self, seed):
        self.x = (seed << 16) | 0x330E

    def lrand(self):
        self.x = (0x5DEECE66D * self.x + 0xB) & ((1 << 48) - 1)
        return self.x >> 17


class Case:
    """status; l_pac, pac (the packed bases, (l_pac + 3) // 4 bytes), cnt[4], n_amb; contigs: (header begin, header end, offset, length, holes);
    holes: (offset, length, byte); headers: the text between '>' and its '\\n'.  kind[i]: what byte i is -- b'>' opens a header, b'H' header
    text, b'E' the '\\n' that closes one, b'S' skipped, b'B' a base; hole[i]: the hole of an ambiguous base or -1; lpos[i]: the bases before i"""

    def __init__(self, text):
        t = self.text = bytes(text)
        rng = Rand48(11)
        codes, contigs, holes, headers = [], [], [], []
        kind, hole, lpos = bytearray(len(t)), [-1] * len(t), [0] * len(t)
        in_hdr, hdr_b, last, n_amb, bad = False, 0, None, 0, False
        for i, b in enumerate(t):
            lpos[i] = len(codes)
            if in_hdr:
                if b == 0x0A:
                    in_hdr, last = False, None
                    headers.append(t[hdr_b:i])
                    contigs.append([hdr_b, i, len(codes), 0, 0])
                    kind[i] = ord("E")
                else:
                    kind[i] = ord("H")
                continue
            if b == 0x3E:
                in_hdr, hdr_b = True, i + 1
                kind[i] = ord(">")
                continue
            if b in BLANKS:
                kind[i] = ord("S")
                continue
            kind[i] = ord("B")
            if not contigs:
                bad = True
                break
            c = nt4(b)
            if c >= 4:
                if last == b:
                    holes[-1][1] += 1
                else:
                    holes.append([len(codes), 1, b])
                    contigs[-1][4] += 1
                hole[i] = len(holes) - 1
                c = rng.lrand() & 3
                n_amb += 1
            last = b
            codes.append(c)
            contigs[-1][3] += 1
        self.kind, self.hole, self.lpos = bytes(kind), hole, lpos
        self.status = BAD_START if bad else EMPTY if not codes else OK
        self.l_pac, self.n_amb = len(codes), n_amb
        self.contigs, self.holes, self.headers = [tuple(c) for c in contigs], [tuple(h) for h in holes], headers
        self.cnt = [codes.count(k) for k in range(4)]
        padded = codes + [0] * (-len(codes) % 4)
        self.pac = bytes(padded[k] << 6 | padded[k + 1] << 4 | padded[k + 2] << 2 | padded[k + 3] for k in range(0, len(padded), 4))

    # ---- the three files
    def pac_file(self):
        return self.pac + (b"\0" if self.l_pac % 4 == 0 else b"") + bytes([self.l_pac % 4])

    def names(self):
        out = []
        for h in self.headers:
            h = h.rstrip(b"\r")
            k = 0
            while k < len(h) and h[k] not in b" \t":
                k += 1
            name, rest = h[:k], h[k:].lstrip(b" \t")
            out.append((name, rest if rest else b"(null)"))
        return out

    def ann_file(self):
        s = b"%d %d 11\n" % (self.l_pac, len(self.contigs))
        for (name, anno), c in zip(self.names(), self.contigs):
            s += b"0 " + name + b" " + anno + b"\n" + b"%d %d %d\n" % (c[2], c[3], c[4])
        return s

    def amb_file(self):
        s = b"%d %d %d\n" % (self.l_pac, len(self.contigs), len(self.holes))
        for off, n, b in self.holes:
            s += b"%d %d %c\n" % (off, n, b)
        return s

    def well_formed(self):
        """what the reference's kseq reads as this project does: '\\n' line ends, '>' at line starts only, no blanks in sequence lines, every
        header closed and followed by bases, names not empty, one space at most between two words of a header, printable ASCII only"""
        t = self.text
        if self.status != OK or not t.startswith(b">") or not t.endswith(b"\n") or b"\r" in t or b"\t" in t or b"\n\n" in t:
            return False
        lines = t[:-1].split(b"\n")
        for k, ln in enumerate(lines):
            if ln[:1] == b">":
                h = ln[1:]
                if not h or h[:1] == b" " or h[-1:] == b" " or b"  " in h or b">" in h or k + 1 == len(lines) or lines[k + 1][:1] == b">" or not all(32 <= b < 127 for b in h):
                    return False
            elif b">" in ln or not all(32 < b < 127 for b in ln):
                return False
        return True

    def cuts(self, window=64):
        """the places (names) at which the cuts of `window`-byte windows fall"""
        t, k, found = self.text, self.kind, set()
        nxt = [None] * (len(t) + 1)                  # the next base at or behind i
        for i in range(len(t) - 1, -1, -1):
            nxt[i] = i if k[i:i + 1] == b"B" else nxt[i + 1]
        prv, p = [None] * (len(t) + 1), None         # the last base before i
        for i in range(len(t)):
            prv[i] = p
            if k[i:i + 1] == b"B":
                p = i
        for c in range(window, len(t), window):
            a, b = k[c - 1:c], k[c:c + 1]
            if a == b"H" and b in (b"H", b"E"):
                found.add("header")
            if a == b">":
                found.add("behind_gt")
            if t[c - 1:c] == b"\r" and t[c:c + 1] == b"\n":
                found.add("cr_lf")
            if a == b"B" and b == b"B":
                found.add("pac%d" % (self.lpos[c] % 4))
                if self.hole[c] >= 0 and self.hole[c] == self.hole[c - 1]:
                    found.add("hole")
            if a == b"S" and b == b"S" and prv[c] is not None and nxt[c] is not None and self.hole[nxt[c]] >= 0 and self.hole[nxt[c]] == self.hole[prv[c]]:
                found.add("hole_blanks")
        return found


CUT_PLACES = {"header", "behind_gt", "cr_lf", "hole", "hole_blanks", "pac0", "pac1", "pac2", "pac3"}


def _bases(n, seed=1, amb=()):
    """n bases, seeded; amb: (position, length, byte) runs written over them"""
    rng = np.random.default_rng(seed)
    s = bytearray(b"ACGTacgt"[int(x)] for x in rng.integers(0, 8, size=n))
    for at, ln, b in amb:
        s[at:at + ln] = bytes([b]) * ln
    return bytes(s)


def _lines(seq, width=60, end=b"\n"):
    return b"".join(seq[k:k + width] + end for k in range(0, len(seq), width))


def _many(n_contigs=40, seed=17):
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n_contigs):
        n = int(rng.integers(900, 2100))
        runs = []
        for _ in range(int(rng.integers(1, 7))):
            runs.append((int(rng.integers(0, n - 401)), int(rng.integers(1, 401)), b"NNNnRY"[int(rng.integers(0, 6))]))
        out.append(b">contig%d some text %d\n" % (c, c) + _lines(_bases(n, seed + 1 + c, runs), 70))
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}

    def add(name, text):
        c[name] = Case(text)

    add("simple", b">a\nACGTACGT\nACG\n")
    add("gt_mid_line", b">a\nACGT>b x\nGGCC\n")
    add("gt_in_header", b">a >b >c\nACGT\n")
    add("cut_header", b">a\nACGT\n>b unfinished")
    add("cut_header_only", b">b unfinished")
    add("cut_header_bare", b">a\nAC\n>")
    add("two_headers", b">a\n>b\nACGT\n>c\n>d\n")
    add("crlf", b">a c\r\nACGT\r\nAC\r\n>b\r\r\r\nGG\r\n")
    add("no_comment", b">name\nACGT\n")
    add("tabs", b">name\t\t two  words\t\nACGT\n>n2 \t\nAC\n")
    add("empty_name", b">\nACGT\n> only comment\nAC\n")
    add("blanks_in_seq", b">a\nAC GT\tAC\n \t\nG G\n")
    add("high_bytes", b">a\xff\x80 c\xfe\nAC\x80\x80\xffGT\xff\n")
    add("dash", b">a\nAC--GT-\n")
    add("n_lower", b">a\nACNnGT\n")
    add("n_newline", b">a\nACN\nNGT\n")
    add("n_blank", b">a\nACN NGT\n")
    add("n_contigs", b">a\nACNN\n>c\nNNGT\n")
    add("n_contigs_mid", b">a\nACNN>c\nNNGT\n")
    add("hole_first_last", b">a\nNNACGTNN\n>b\nNACN\n")
    add("all_n", b">a\nNNNNN\nNNNN\n")
    for r in range(4):
        add("lpac%d" % r, b">a\n" + _bases(8 + r, 3 + r) + b"\n")
    add("bad_start", b"ACGT\n>a\nACGT\n")
    add("bad_start_blank", b" \n\tA>a\nACGT\n")
    add("blanks_only", b" \n\r\t\n")
    add("headers_only", b">a\n>b\n")
    add("empty", b"")
    add("single_line", b">long one\n" + _bases(5000, 5, ((700, 900, 0x4E), (4990, 10, 0x6E))) + b"\n")
    add("hdr300", b">" + b"h" * 150 + b" " + b"c" * 148 + b"\nACGTN\n")
    # the window cuts, at 64 bytes
    add("cut_behind_gt", b">a\n" + _bases(60, 7) + b">b\n" + _bases(70, 8) + b"\n")
    add("cut_cr_lf", b">a\r\n" + _bases(59, 9) + b"\r\n" + _bases(30, 10) + b"\r\n")
    add("cut_hole", b">a\n" + _bases(50, 11) + b"N" * 30 + _bases(20, 12) + b"\n")
    add("cut_hole_blanks", b">a\n" + _bases(55, 13) + b"NNNN\n \t\nNNNN" + _bases(10, 14) + b"\n")
    for k in range(1, 5):
        add("cut_pac_%d" % k, b">" + b"x" * k + b"\n" + _bases(130, 20 + k, ((90, 7, 0x4E),)) + b"\n")
    add("many", _many())
    return c


SMALL = tuple(n for n in cases() if n != "many")


def check_cases():
    cs = cases()
    for name, c in cs.items():
        assert name == "many" or len(c.text) <= 5100, name
    assert cs["gt_mid_line"].headers == [b"a", b"b x"] and cs["gt_mid_line"].contigs[1][2] == 4
    assert cs["gt_in_header"].headers == [b"a >b >c"] and len(cs["gt_in_header"].contigs) == 1
    assert len(cs["cut_header"].contigs) == 1 and cs["cut_header"].status == OK and cs["cut_header_only"].status == EMPTY and not cs["cut_header_only"].contigs
    assert len(cs["cut_header_bare"].contigs) == 1 and cs["cut_header_bare"].l_pac == 2
    assert [x[3] for x in cs["two_headers"].contigs] == [0, 4, 0, 0]
    assert cs["crlf"].names() == [(b"a", b"c"), (b"b", b"(null)")] and cs["crlf"].headers[1] == b"b\r\r\r" and cs["crlf"].l_pac == 8
    assert cs["no_comment"].names() == [(b"name", b"(null)")]
    assert cs["tabs"].names() == [(b"name", b"two  words\t"), (b"n2", b"(null)")]
    assert cs["empty_name"].names() == [(b"", b"(null)"), (b"", b"only comment")]
    assert cs["blanks_in_seq"].l_pac == 8 and not cs["blanks_in_seq"].holes
    assert cs["high_bytes"].holes == [(2, 2, 0x80), (4, 1, 0xFF), (7, 1, 0xFF)] and cs["high_bytes"].l_pac == 8
    assert cs["dash"].holes == [(2, 2, 0x2D), (6, 1, 0x2D)]
    assert cs["n_lower"].holes == [(2, 1, 0x4E), (3, 1, 0x6E)]
    assert cs["n_newline"].holes == [(2, 2, 0x4E)] and cs["n_blank"].holes == [(2, 2, 0x4E)]
    for name in ("n_contigs", "n_contigs_mid"):
        assert cs[name].holes == [(2, 2, 0x4E), (4, 2, 0x4E)] and [x[4] for x in cs[name].contigs] == [1, 1], name
    assert cs["hole_first_last"].holes == [(0, 2, 0x4E), (6, 2, 0x4E), (8, 1, 0x4E), (11, 1, 0x4E)]
    assert cs["all_n"].n_amb == cs["all_n"].l_pac == 9 and len(cs["all_n"].holes) == 1
    assert [cs["lpac%d" % r].l_pac % 4 for r in range(4)] == [0, 1, 2, 3]
    assert len(cs["lpac0"].pac_file()) == cs["lpac0"].l_pac // 4 + 2 and len(cs["lpac1"].pac_file()) == cs["lpac1"].l_pac // 4 + 2
    assert cs["bad_start"].status == BAD_START and cs["bad_start_blank"].status == BAD_START
    assert cs["blanks_only"].status == EMPTY and cs["empty"].status == EMPTY and cs["headers_only"].status == EMPTY
    assert cs["single_line"].l_pac == 5000 and cs["single_line"].text.count(b"\n") == 2 and cs["single_line"].holes[-1] == (4990, 10, 0x6E)
    assert len(cs["hdr300"].headers[0]) == 299 and len(cs["hdr300"].text) > 300
    m = cs["many"]
    assert len(m.contigs) == 40 and 50_000 < m.l_pac < 70_000 and m.n_amb > 1 << 12 and any(h[2] == 0x6E for h in m.holes) and max(h[1] for h in m.holes) > 300
    # the first numbers of srand48(11)'s stream, as glibc gives them
    r = Rand48(11)
    assert [r.lrand() for _ in range(3)] == [1609868485, 1074594562, 470884846]
    found = set()
    for c in cs.values():
        if c.status == OK:
            found |= c.cuts(64)
    assert found == CUT_PLACES, sorted(CUT_PLACES - found)
    assert sum(c.well_formed() for c in cs.values()) >= 10 and cs["many"].well_formed() and not cs["crlf"].well_formed() and not cs["gt_mid_line"].well_formed()

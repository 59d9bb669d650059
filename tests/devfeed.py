"""Helpers of tests/test_device_feeder.py: FASTQ texts (the recipe of tests/test_feeder.py rebuilt, a fast one for long runs, a seeded
generator of damaged files), raw snapshots of an arx_super_batch, the comparison with the restatement (oracle/fastq_reader.py), an
independent walk over the lines for the conditions the tests assert, a raw BAM record reader."""
import ctypes as C
import gzip
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import fastq_reader  # noqa: E402

from arachne_amd import api  # noqa: E402

SIM = os.path.join(HERE, "hostsim", "libarx_hostsim.so")
ACGT = "ACGTN"
DEFAULT_CHUNK = 8 << 20          # include/arachne_amd.h: arx_feeder_open_device, chunk_bytes = 0


def fastq(groups, seed=0, read_len=40):
    """groups: list of (barcode or None, n_records) -> (r1_text, r2_text); the recipe of tests/test_feeder.py"""
    rng = np.random.default_rng(seed)
    r1, r2 = [], []
    k = 0
    for bc, n in groups:
        for _ in range(n):
            s1 = "".join(ACGT[x] for x in rng.integers(0, 5, size=read_len))
            s2 = "".join(ACGT[x] for x in rng.integers(0, 4, size=read_len - 3))
            q1 = "".join(chr(33 + x) for x in rng.integers(0, 40, size=read_len))
            q2 = "".join(chr(33 + x) for x in rng.integers(0, 40, size=read_len - 3))
            tags = "" if bc is None else f"\tBX:Z:{bc}\tVX:i:{k % 2}"
            r1.append(f"@read{k}/1{tags}\n{s1}\n+\n{q1}\n")
            r2.append(f"@read{k}/2{tags}\n{s2}\n+\n{q2}\n")
            k += 1
    return "".join(r1), "".join(r2)


def fastq_long_runs(groups, seed=1, read_len=24):
    """the same shape for runs of tens of thousands of records: sequences and qualities are windows of one random text"""
    rng = np.random.default_rng(seed)
    pool_s = "".join(ACGT[x] for x in rng.integers(0, 5, size=4096))
    pool_q = "".join(chr(33 + x) for x in rng.integers(0, 40, size=4096))
    r1, r2 = [], []
    k = 0
    for bc, n in groups:
        for _ in range(n):
            a = (k * 7919) % (4096 - read_len)
            r1.append(f"@read{k}/1\tBX:Z:{bc}\tVX:i:{k % 2}\n{pool_s[a:a + read_len]}\n+\n{pool_q[a:a + read_len]}\n")
            r2.append(f"@read{k}/2\n{pool_s[a + 1:a + read_len - 2]}\n+\n{pool_q[a + 1:a + read_len - 2]}\n")
            k += 1
    return "".join(r1), "".join(r2)


def write(d, name, text, gz=False):
    data = text if isinstance(text, bytes) else text.encode("latin-1")
    p = os.path.join(d, name)
    with (gzip.open(p, "wb") if gz else open(p, "wb")) as f:
        f.write(data)
    return p


def snapshot(sb, n_sets):
    """every array of an arx_super_batch as bytes, read where the feeder keeps it"""
    P = int(sb.n_pairs)
    out = dict(n_sets=int(n_sets), n_pairs=P, bad_lines=int(sb.bad_lines))

    def raw(ptr, nbytes):
        return C.string_at(ptr, nbytes) if nbytes else b""
    out["lens"] = raw(sb.lens, 8 * P)
    nb = int(np.frombuffer(out["lens"], np.int32).sum(dtype=np.int64))
    out["set_pair_off"], out["unique"], out["do_rfa"] = raw(sb.set_pair_off, 8 * (n_sets + 1)), raw(sb.unique, n_sets), raw(sb.do_rfa, n_sets)
    out["bases"], out["quals"], out["valid"] = raw(sb.bases, nb), raw(sb.quals, nb), raw(sb.valid, P)
    for off, dat, n in (("name_off", "names", P), ("rg_off", "rgs", P), ("barcode_off", "barcodes", n_sets)):
        out[off] = raw(getattr(sb, off), 8 * (n + 1))
        out[dat] = raw(getattr(sb, dat), int(np.frombuffer(out[off], np.int64)[-1]))
    return out


def feed_all(fd, target, each=None):
    """every super-batch of a feeder as a snapshot; each(fd, sb, snap) is called while the arrays are valid"""
    out = []
    while True:
        sb = api._SuperBatch()
        n = fd.lib.arx_feeder_next(fd.h, int(target), C.byref(sb))
        assert n >= 0
        if n == 0:
            break
        out.append(snapshot(sb, n))
        if each:
            each(fd, sb, out[-1])
    sb = api._SuperBatch()
    assert fd.lib.arx_feeder_next(fd.h, int(target), C.byref(sb)) == 0           # stays at the end
    out.append(dict(n_sets=0, bad_lines=int(sb.bad_lines)))
    return out


def assert_same_batches(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.keys() == b.keys()
        for key in a:
            assert a[key] == b[key], (k, key)


def nt4(ch):
    return "ACGT".find(ch.upper()) if ch.upper() in "ACGT" else 4


def check_against_restatement(batches, r1_text, r2_text):
    """set sizes, flags, barcodes and every record against oracle/fastq_reader.all_sets; the quality strings cut or padded with '!' to the
    sequence as append_read (feeder.h) does"""
    sets, bad = fastq_reader.all_sets(r1_text, r2_text)
    k = 0
    for sb in batches:
        if sb["n_sets"] == 0:
            continue
        lens = np.frombuffer(sb["lens"], np.int32)
        boff = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
        spo, noff, goff, coff = (np.frombuffer(sb[x], np.int64) for x in ("set_pair_off", "name_off", "rg_off", "barcode_off"))
        for s in range(sb["n_sets"]):
            recs, unique, rfa = sets[k]
            k += 1
            p0, p1 = int(spo[s]), int(spo[s + 1])
            assert p1 - p0 == len(recs), (k, p1 - p0, len(recs))
            assert (bool(sb["unique"][s]), bool(sb["do_rfa"][s])) == (unique, rfa)
            assert sb["barcodes"][coff[s]:coff[s + 1]].decode("latin-1") == recs[0]["barcode"]
            for j, rec in enumerate(recs):
                p = p0 + j
                assert sb["names"][noff[p]:noff[p + 1]].decode("latin-1") == rec["info"]
                assert sb["rgs"][goff[p]:goff[p + 1]].decode("latin-1") == rec["rg"]
                assert bool(sb["valid"][p]) == rec["valid"]
                for side, (sq, ql) in enumerate(((rec["s1"], rec["q1"]), (rec["s2"], rec["q2"]))):
                    a, b = int(boff[2 * p + side]), int(boff[2 * p + side + 1])
                    assert b - a == len(sq)
                    assert list(sb["bases"][a:b]) == [nt4(c) for c in sq]
                    assert sb["quals"][a:b].decode("latin-1") == (ql + "!" * len(sq))[:len(sq)]
    assert k == len(sets)
    assert batches[-1]["bad_lines"] == bad
    return sets, bad


def walk(r1_text, r2_text):
    """Feeder::read_one's walk restated on line lists, for the conditions the tests assert: -> (header line indices, skipped line indices).
    Lines exist only where both files have a '\\n'-terminated one."""
    l1, l2 = r1_text.split("\n")[:-1], r2_text.split("\n")[:-1]
    n = min(len(l1), len(l2))
    heads, bad, j = [], [], 0
    while j < n:
        if l1[j][:1] == "@":
            heads.append(j)
            j += 4
        else:
            bad.append(j)
            j += 1
    return heads, bad


def damaged_pair(seed):
    """A small file pair with, drawn per record: a stray line between records, a quality line that starts with '@', an empty line, CRLF
    ends, a quality line shorter / longer than its sequence, a header of one field, BX last on the line, `BX:Z:` followed by white space,
    two BX tags, VX:i:2, lower-case and IUPAC bases, a record without its '+' line (everything behind it is then read out of step); per
    file: unequal line counts, end of input after 1, 2 or 3 lines of a record, no final newline.
    -> (r1_text, r2_text, info): info["at_qual"] = R1 line indices of the quality lines that start with '@', info["unequal"]"""
    rng = np.random.default_rng(1000 + seed)
    n_rec = int(rng.integers(4, 22))
    pool = ["A-1", "B-7", "CC", "D-1-2"]
    bases = "ACGTacgtNnRYKMSWryk"
    f1, f2 = [], []                     # lists of lines (without their ends), and the end of each line
    at_qual = []
    bc = pool[int(rng.integers(len(pool)))]
    shifted = False
    force_at = False
    for k in range(n_rec):
        if rng.random() < 0.35:
            bc = pool[int(rng.integers(len(pool)))]
        end = "\r\n" if rng.random() < 0.1 else "\n"
        if rng.random() < 0.15:
            f1.append("stray line %d" % k + end); f2.append("other stray" + end)
        if rng.random() < 0.1:
            f1.append(end); f2.append("\n")                       # an empty line (a lone '\r' where the record has CRLF ends)
        L1, L2 = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        lower = rng.random() < 0.2
        s1 = "".join((bases if lower else "ACGT")[int(x)] for x in rng.integers(0, len(bases) if lower else 4, size=L1))
        s2 = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=L2))
        q1 = "".join(chr(35 + int(x)) for x in rng.integers(0, 29, size=L1))   # '#' .. '?': never '@' by chance
        q2 = "".join(chr(35 + int(x)) for x in rng.integers(0, 29, size=L2))
        u = rng.random()
        if u < 0.15:
            q1 = q1[:max(1, L1 // 2)]
        elif u < 0.3:
            q1 = q1 + "IIII"
        if rng.random() < 0.15:
            q2 = q2[:-1] if rng.random() < 0.5 else q2 + "J"
        if force_at or rng.random() < 0.2:
            q1 = "@" + (q1[1:] or "#")                          # never '@' alone: read as a header it must hold a non-space byte
        force_at = False
        sep = [" ", "\t", "  ", " \t", "\v", "\f"][int(rng.integers(6))]
        vx = "VX:i:%d" % int(rng.integers(0, 2))
        form = rng.random()
        name = "r%d/1" % k
        if form < 0.1:
            h1 = name                                           # one field: no barcode, empty ReadGroupId
        elif form < 0.25:
            h1 = name + sep + vx + sep + "BX:Z:" + bc           # BX last on the line
        elif form < 0.35:
            h1 = name + sep + "BX:Z:" + sep + vx                # BX:Z: followed by white space: no barcode
        elif form < 0.45:
            h1 = name + sep + "BX:Z:" + bc + sep + "BX:Z:other-9" + sep + vx
        elif form < 0.55:
            h1 = name + sep + "BX:Z:" + bc + sep + "VX:i:2"
        elif form < 0.6:
            h1 = " " + name + sep + "BX:Z:" + bc + sep + vx + " "
        else:
            h1 = name + sep + "BX:Z:" + bc + sep + vx
        rec1 = ["@" + h1, s1, "+", q1]
        rec2 = ["@r%d/2" % k, s2, "+", q2]
        if not shifted and k < n_rec - 2 and rng.random() < 0.12:   # the '+' line is missing in both files: the next header is passed unseen
            del rec1[2], rec2[2]
            shifted = True
            force_at = rng.random() < 0.8
        if rec1[-1][:1] == "@":
            at_qual.append(len(f1) + len(rec1) - 1)
        f1 += [x + end for x in rec1]
        f2 += [x + end for x in rec2]
    unequal = False
    u = rng.random()
    if u < 0.15:
        f2 = f2[:len(f2) - int(rng.integers(1, 6))]; unequal = True
    elif u < 0.3:
        f1 = f1[:len(f1) - int(rng.integers(1, 6))]; unequal = True
    elif u < 0.4:
        f1 += ["@extra/1 BX:Z:Z-9\n", "ACGT\n", "+\n", "IIII\n"]; unequal = True
    elif u < 0.6:                                                  # both files end after 1, 2 or 3 lines of a record
        cut = int(rng.integers(1, 4))
        f1 += ["@tail/1 BX:Z:%s\n" % bc, "ACGT\n", "+\n"][:cut]; f2 += ["@tail/2\n", "TTTT\n", "+\n"][:cut]
    t1, t2 = "".join(f1), "".join(f2)
    if rng.random() < 0.2:
        t1 = t1[:-1]
    if rng.random() < 0.2:
        t2 = t2[:-1]
    return t1, t2, dict(at_qual=at_qual, unequal=unequal and t1.count("\n") != t2.count("\n"))


def copy_home(lib_path, ptr, nbytes):
    """device memory of the feeder's or a batch's library -> bytes (the host test double's "device" memory is host memory)"""
    if nbytes == 0:
        return b""
    if lib_path == SIM:
        return C.string_at(ptr, nbytes)
    hip = None
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            continue
    assert hip is not None, "libamdhip64.so not found"
    buf = C.create_string_buffer(nbytes)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(buf, C.c_void_p(ptr), nbytes, 2) == 0
    return buf.raw


def bam_records(path):
    """the records of a BAM file as raw byte strings (an independent reader: BGZF blocks inflated with zlib, the header skipped)"""
    raw = open(path, "rb").read()
    data, o = [], 0
    while o < len(raw):
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        data.append(zlib.decompress(raw[o + 18:o + bsize - 8], -15))
        o += bsize
    data = b"".join(data)
    l_text = struct.unpack_from("<i", data, 4)[0]
    o = 8 + l_text
    n_ref = struct.unpack_from("<i", data, o)[0]; o += 4
    for _ in range(n_ref):
        o += 4 + struct.unpack_from("<i", data, o)[0] + 4
    recs = []
    while o < len(data):
        bs = struct.unpack_from("<i", data, o)[0]
        recs.append(data[o + 4:o + 4 + bs])
        o += 4 + bs
    return recs

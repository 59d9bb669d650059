#!/usr/bin/env python3
"""The header standardization of a FASTQ file pair on the GPU (arx_fastq_standardize) beside the sort that follows it (arx_fastq_sort).

One synthetic file pair of --pairs pairs from arachne_amd/synth.py (a small genome, --per-barcode pairs a barcode, 2x150 bp), its headers put
into raw TELLseq form (`@r<pair>:<18 letters>`, every 16th barcode with an N), as plain text and as BGZF (blocks of 65,280 bytes, level 1),
files in the page cache.  One JSON line per measurement:
  input         the sizes
  standardize   raw -> standardized        sort   standardized -> sorted         (what; arm: plain -> plain, or bgzf -> BGZF)
--repeats times alternating, untimed (the call's seconds and pairs/s; phases by wall clock), then once each with the TIMED flag (every launch
group awaited).  The first standardized output of each arm is compared with the restatement of tests/fqstdcases.py.
  summary       per arm the two series, the sort's spread (max - min) and whether the standardization's median exceeds the sort's by more
Usage: fastq_standardize_bench.py [--pairs 1000000] [--per-barcode 200] [--repeats 5] [--out-dir DIR]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bgzfio  # noqa: E402  (tests/bgzfio.py: the BGZF writer)
import fqsortcases as fc  # noqa: E402
import fqstdcases as sc  # noqa: E402  (the restatement the output is held to)
from arachne_amd import api, synth  # noqa: E402

STD_PHASES = ("read", "inflate", "parse", "fields", "compose", "compress", "write")
SORT_PHASES = ("read", "inflate", "parse", "keys", "sort", "gather", "compress", "write")


def write_bgzf(path, text):
    with open(path, "wb") as g:
        for a in range(0, len(text), 256 * bgzfio.BLOCK_IN):
            g.write(bgzfio.write_bgzf(text[a:a + 256 * bgzfio.BLOCK_IN], level=1, eof=False))
        g.write(bgzfio.EOF_BLOCK)


def tell_code(k):
    """barcode number k as 18 letters, ascending with k; every 16th holds an N"""
    s = bytes(b"ACGT"[(k >> (2 * (17 - i))) & 3] for i in range(18))
    return s[:17] + b"N" if k % 16 == 15 else s


def raw_tellseq(text, codes):
    """the standard headers of a synth file -> raw TELLseq ones; codes: barcode string -> letters"""
    lines = text.split(b"\n")
    for j in range(0, len(lines) - 1, 4):
        name = lines[j].split(b"\t", 1)[0]
        lines[j] = name[:-2] + b":" + codes[fc.barcode(lines[j])]
    return b"\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--per-barcode", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out-dir", default=None)
    args = ap.parse_args()
    d = args.out_dir or tempfile.mkdtemp(prefix="arx_fqstd_bench_")
    os.makedirs(d, exist_ok=True)
    g = synth.make_genome(21, [2_000_000], fast=True)
    rs = synth.make_reads(22, g, max(1, args.pairs // args.per_barcode), args.per_barcode, fast=True)
    s1, s2 = os.path.join(d, "synth1.fq"), os.path.join(d, "synth2.fq")
    synth.write_fastq_fast(rs, s1, s2)
    t1 = open(s1, "rb").read()
    codes = {b: tell_code(k) for k, b in enumerate(dict.fromkeys(fc.barcode(h) for h in t1.split(b"\n")[0::4] if h))}
    texts = (raw_tellseq(t1, codes), raw_tellseq(open(s2, "rb").read(), codes))
    del t1
    plain = (os.path.join(d, "raw1.fq"), os.path.join(d, "raw2.fq"))
    bz = tuple(p + ".gz" for p in plain)
    for p, q, t in zip(plain, bz, texts):
        with open(p, "wb") as f:
            f.write(t)
        write_bgzf(q, t)
    n = texts[0].count(b"\n") // 4
    want = None
    for p in plain + bz:                                         # into the page cache
        with open(p, "rb") as f:
            while f.read(1 << 24):
                pass
    print(json.dumps(dict(what="input", pairs=n, barcodes=len(codes), plain_bytes=sum(os.path.getsize(p) for p in plain), bgzf_bytes=sum(os.path.getsize(p) for p in bz))), flush=True)
    summary = {}
    for arm, src, bgzf in (("plain", plain, False), ("bgzf", bz, True)):
        ext = ".gz" if bgzf else ""
        std = (os.path.join(d, "std1.fq" + ext), os.path.join(d, "std2.fq" + ext))
        out = (os.path.join(d, "out1.fq" + ext), os.path.join(d, "out2.fq" + ext))
        series = dict(standardize=[], sort=[])
        for rep in range(args.repeats + 1):
            timed = rep == args.repeats
            for what in ("standardize", "sort"):
                t = time.time()
                if what == "standardize":
                    st = api.fastq_standardize(*src, *std, format="auto", bgzf=bgzf, timed=timed)
                    phases = STD_PHASES
                else:
                    st = api.fastq_sort(*std, *out, bgzf=bgzf, timed=timed)
                    phases = SORT_PHASES
                s = time.time() - t
                row = dict(what=what, arm=arm, timed=timed, seconds=round(s, 4), pairs_per_s=round(n / s), records=st["records"], windows=st["windows"], slabs=st["slabs"],
                           **{p + "_ms": round(st[p + "_us"] / 1e3, 2) for p in phases})
                if what == "standardize":
                    row.update(format=st["format"], with_barcode=st["with_barcode"], valid=st["valid"])
                    if rep == 0:
                        got = [open(p, "rb").read() for p in std]
                        if bgzf:
                            row["out_bytes"] = sum(len(x) for x in got)
                            got = [bgzfio.inflate(x) for x in got]
                        if want is None:
                            c = sc.Case(*texts)
                            want = (c.out1, c.out2, c.with_bc, c.valid)
                            del c
                        row["output_is_the_restatement"] = got[0] == want[0] and got[1] == want[1] and (st["with_barcode"], st["valid"]) == want[2:]
                        del got
                if not timed:
                    series[what].append(round(s, 4))
                print(json.dumps(row), flush=True)
        spread = max(series["sort"]) - min(series["sort"])
        ms, mo = statistics.median(series["standardize"]), statistics.median(series["sort"])
        summary[arm] = dict(standardize_s=series["standardize"], sort_s=series["sort"], sort_spread_s=round(spread, 4), standardize_median_s=ms, sort_median_s=mo,
                            standardize_within_sort_plus_spread=ms <= mo + spread)
    print(json.dumps(dict(what="summary", **summary)), flush=True)
    if not args.out_dir:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

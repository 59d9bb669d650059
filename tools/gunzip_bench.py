#!/usr/bin/env python3
"""Plain gzip FASTQ input inflated on the GPU in chunks (ARX_FQSORT_GUNZIP_DEVICE) against zlib on the reader threads, which is what the
file-pair calls do without the flag.

One synthetic file pair of --pairs pairs from arachne_amd/synth.py (the read set the other FASTQ tools use: --per-barcode pairs a barcode,
2x150 bp, written by synth.write_fastq_fast) as ordinary gzip files, one member each, zlib level --level; files in the page cache.  One JSON
line per measurement:
  input      the sizes
  zlib       one Python zlib.decompress of R1 (one thread), for scale
  selftest   arx_selftest_gunzip of R1 alone at every --chunk-kib: seconds end to end (upload, launches, text home) and the microseconds of
             the phases -- find, decode, windows and resolve -- with the launch and chunk counts and whether the host had to take over
  prepare    arx_fastq_prepare of the pair, gunzip="host" and gunzip="device" alternating, --repeats passes each, outputs plain
  sort       arx_fastq_sort of the pair, the same way
The first output of every device arm is compared with the host arm's.
Usage: gunzip_bench.py [--pairs 1000000] [--per-barcode 77] [--level 1] [--repeats 3] [--chunk-kib 32,64,128] [--out-dir DIR] [--jsonl FILE]
Every line is appended to --jsonl (default: profiles/device_gunzip/gunzip_bench.jsonl) as well as printed."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from arachne_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--per-barcode", type=int, default=77)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk-kib", default="32,64,128")
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--jsonl", default=os.path.join(ROOT, "profiles", "device_gunzip", "gunzip_bench.jsonl"))
    args = ap.parse_args()
    d = args.out_dir or tempfile.mkdtemp(prefix="arx_gunzip_bench_")
    os.makedirs(d, exist_ok=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.jsonl)), exist_ok=True)
    log = open(args.jsonl, "a")

    def say(**row):
        line = json.dumps(row)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    g = synth.make_genome(21, [2_000_000], fast=True)
    rs = synth.make_reads(22, g, max(1, args.pairs // args.per_barcode), args.per_barcode, fast=True)
    plain = (os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq"))
    synth.write_fastq_fast(rs, *plain)
    gz = tuple(p + ".gz" for p in plain)
    n_text = []
    for p, q in zip(plain, gz):
        text = open(p, "rb").read()
        n_text.append(len(text))
        z = zlib.compressobj(args.level, zlib.DEFLATED, 31)
        with open(q, "wb") as f:
            for a in range(0, len(text), 1 << 24):
                f.write(z.compress(text[a:a + (1 << 24)]))
            f.write(z.flush())
    n = text.count(b"\n") // 4
    del text
    for p in gz:                                                 # into the page cache
        with open(p, "rb") as f:
            while f.read(1 << 24):
                pass
    say(what="input", pairs=n, level=args.level, plain_bytes=sum(n_text), gzip_bytes=sum(os.path.getsize(p) for p in gz))
    comp = open(gz[0], "rb").read()
    t = time.time()
    want = zlib.decompress(comp, 31)
    say(what="zlib", seconds=round(time.time() - t, 4), gb_per_s=round(len(want) / (time.time() - t) / 1e9, 3))
    for kib in (int(x) for x in args.chunk_kib.split(",") if x.strip()):
        for rep in range(args.repeats):
            t = time.time()
            r = api.selftest_gunzip(comp, chunk_bytes=kib << 10, cap=len(want) + 64)
            s = time.time() - t
            dev_us = r["us_find"] + r["us_decode"] + r["us_resolve"]
            say(what="selftest", chunk_kib=kib, seconds=round(s, 4), same_bytes=r["out"] == want, device_ms=round(dev_us / 1e3, 2),
                device_gb_per_s=round(len(want) / max(dev_us, 1) / 1e3, 3), **{k: r[k] for k in api.GUNZIP_STATS})
    del comp, want
    out = {how: (os.path.join(d, "out1_%s.fq" % how), os.path.join(d, "out2_%s.fq" % how)) for how in ("host", "device")}
    for what, call in (("prepare", api.fastq_prepare), ("sort", api.fastq_sort)):
        for rep in range(args.repeats):
            for how in ("host", "device"):
                t = time.time()
                st = call(*gz, *out[how], gunzip=how)
                s = time.time() - t
                row = dict(what=what, gunzip=how, seconds=round(s, 4), pairs_per_s=round(n / s), records=st["records"], read_ms=round(st["read_us"] / 1e3, 2),
                           inflate_ms=round(st["inflate_us"] / 1e3, 2))
                if rep == 0 and how == "device":
                    row["same_files_as_host"] = all(open(a, "rb").read() == open(b, "rb").read() for a, b in zip(out["host"], out["device"]))
                say(**row)
    if not args.out_dir:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

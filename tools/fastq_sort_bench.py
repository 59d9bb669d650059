#!/usr/bin/env python3
"""The sort of a FASTQ file pair by barcode on the GPU (arx_fastq_sort), phase by phase.

One synthetic file pair of --pairs pairs from arachne_amd/synth.py (a small genome, --per-barcode pairs a barcode, 2x150 bp, written by
synth.write_fastq_fast), shuffled at record level by a seeded permutation that keeps the order inside every barcode, as plain text and as
BGZF (blocks of 65,280 bytes, level 1), files in the page cache.  One JSON line per measurement:
  input        the sizes
  plain        plain -> plain          bgzf   BGZF -> BGZF          check   ARX_FQSORT_CHECK on the plain and on the BGZF pair
each --repeats times untimed (the call's seconds and pairs/s; phases by wall clock) and once with ARX_FQSORT_TIMED (every launch group awaited:
read, inflate, parse, keys, sort, gather, compress, write in ms).  The first sorted output is compared with Python's stable sort of the records.
--run-bytes takes a comma-separated list: 0 is the in-core call above, any other value repeats the plain and the bgzf arm through
arx_fastq_sort_ex with that run size (-1: the library's choice), temporary files in the output directory; those lines carry run_bytes, the
sorted runs, the temporary bytes and the milliseconds spent writing the runs and reading them back.  --also-lib PATH adds the in-core plain arm
of another build of the library (the parent commit's, say), its passes alternated with this tree's (what: plain_this, plain_other).
Usage: fastq_sort_bench.py [--pairs 1000000] [--per-barcode 200] [--repeats 3] [--out-dir DIR] [--run-bytes 0,RB,...] [--also-lib PATH]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import bgzfio  # noqa: E402  (tests/bgzfio.py: the BGZF writer)
import fqsortcases as fc  # noqa: E402  (the restatement the output is held to)
from arachne_amd import api, synth  # noqa: E402

PHASES = ("read", "inflate", "parse", "keys", "sort", "gather", "compress", "write")


def records_of(text):
    lines = text.split(b"\n")[:-1]
    assert len(lines) % 4 == 0
    return [b"\n".join(lines[k:k + 4]) + b"\n" for k in range(0, len(lines), 4)]


def write_bgzf(path, text):
    with open(path, "wb") as g:
        for a in range(0, len(text), 256 * bgzfio.BLOCK_IN):
            g.write(bgzfio.write_bgzf(text[a:a + 256 * bgzfio.BLOCK_IN], level=1, eof=False))
        g.write(bgzfio.EOF_BLOCK)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--per-barcode", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--run-bytes", default="0")
    ap.add_argument("--also-lib", default=None)
    args = ap.parse_args()
    run_sizes = [int(x) for x in args.run_bytes.split(",") if x.strip()]
    d = args.out_dir or tempfile.mkdtemp(prefix="arx_fqsort_bench_")
    os.makedirs(d, exist_ok=True)
    g = synth.make_genome(21, [2_000_000], fast=True)
    rs = synth.make_reads(22, g, max(1, args.pairs // args.per_barcode), args.per_barcode, fast=True)
    s1, s2 = os.path.join(d, "sorted1.fq"), os.path.join(d, "sorted2.fq")
    synth.write_fastq_fast(rs, s1, s2)
    r1, r2 = records_of(open(s1, "rb").read()), records_of(open(s2, "rb").read())
    bcs = [fc.barcode(r.split(b"\n", 1)[0]) for r in r1]
    n = len(r1)
    # the shuffle of tests/test_fastq_sort_gpu.py: a seeded order of the barcodes, every barcode's records in their own order
    perm = np.random.default_rng(23).permutation(n)
    ids = {b: k for k, b in enumerate(dict.fromkeys(bcs))}
    bid = np.array([ids[b] for b in bcs])
    place = np.argsort(bid[perm], kind="stable")                 # the shuffled places of barcode 0, then of barcode 1, ...
    src = np.argsort(bid, kind="stable")                         # the records of barcode 0 in their order, then of barcode 1, ...
    at = np.empty(n, dtype=np.int64)
    at[place] = src
    plain = (os.path.join(d, "shuf1.fq"), os.path.join(d, "shuf2.fq"))
    texts = []
    for p, recs in zip(plain, (r1, r2)):
        t = b"".join(recs[k] for k in at)
        texts.append(t)
        with open(p, "wb") as f:
            f.write(t)
    bz = tuple(p + ".gz" for p in plain)
    for p, t in zip(bz, texts):
        write_bgzf(p, t)
    order = sorted(range(n), key=lambda k: bcs[at[k]])           # stable
    want = tuple(b"".join(recs[at[k]] for k in order) for recs in (r1, r2))
    del r1, r2, texts
    for p in plain + bz:                                         # into the page cache
        with open(p, "rb") as f:
            while f.read(1 << 24):
                pass
    print(json.dumps(dict(what="input", pairs=n, barcodes=len(ids), plain_bytes=sum(os.path.getsize(p) for p in plain), bgzf_bytes=sum(os.path.getsize(p) for p in bz))), flush=True)
    out = (os.path.join(d, "out1.fq"), os.path.join(d, "out2.fq"))
    arms = (("plain", plain, dict(bgzf=False)), ("bgzf", bz, dict(bgzf=True)), ("check_plain", plain, dict(check=True)), ("check_bgzf", bz, dict(check=True)))
    first = True
    for rb in run_sizes:
        for what, src_files, kw in arms:
            if rb != 0 and kw.get("check"):
                continue
            outs = (None, None) if kw.get("check") else out
            for rep in range(args.repeats + 1):
                timed = rep == args.repeats
                t = time.time()
                st = api.fastq_sort(*src_files, *outs, timed=timed, **kw) if rb == 0 else api.fastq_sort_ex(*src_files, *outs, timed=timed, run_bytes=rb, tmp_dir=d, **kw)
                s = time.time() - t
                row = dict(what=what, run_bytes=rb, timed=timed, seconds=round(s, 4), pairs_per_s=round(n / s), records=st["records"], runs=st["runs"], distinct=st["distinct"],
                           sort_passes=st["sort_passes"], windows=st["windows"], slabs=st["slabs"], **{p + "_ms": round(st[p + "_us"] / 1e3, 2) for p in PHASES})
                if rb != 0:
                    row.update(sorted_runs=st["sorted_runs"], tmp_bytes=st["tmp_bytes"], run_write_ms=round(st["run_write_us"] / 1e3, 2), run_read_ms=round(st["run_read_us"] / 1e3, 2))
                if rep == 0 and not kw.get("check"):
                    got = [open(p, "rb").read() for p in out]
                    if kw["bgzf"]:
                        row["out_bytes"] = sum(len(x) for x in got)
                        got = [bgzfio.inflate(x) for x in got]
                    row["output_is_the_stable_sort"] = got[0] == want[0] and got[1] == want[1]
                    if not first:
                        del got
                    first = False
                print(json.dumps(row), flush=True)
    if args.also_lib:
        for rep in range(args.repeats + 1):
            for what, lib in (("plain_this", api.LIB_PATH), ("plain_other", args.also_lib)):
                t = time.time()
                st = api.fastq_sort(*plain, *out, lib_path=lib)
                s = time.time() - t
                print(json.dumps(dict(what=what, run_bytes=0, timed=False, seconds=round(s, 4), pairs_per_s=round(n / s), records=st["records"],
                                      **{p + "_ms": round(st[p + "_us"] / 1e3, 2) for p in PHASES})), flush=True)
    if not args.out_dir:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The fused call (arx_fastq_prepare) beside the two calls it replaces (arx_fastq_standardize, then arx_fastq_sort_ex) on the same raw file pair.

The input is tools/fastq_standardize_bench.py's: one synthetic pair of --pairs pairs from arachne_amd/synth.py (2x150 bp, --per-barcode pairs a
barcode), its headers in raw TELLseq form, as plain text and as BGZF, files in the page cache.  Four arms: plain -> plain and bgzf -> BGZF, each
in core (run_bytes 0) and in runs (--run-bytes of text per file and run).  Per arm --repeats times alternating, untimed: the two calls (the
standardized files between them in the arm's form, as a pipeline would keep them), then the fused call; then once each with the TIMED flag
(every launch group awaited).  The first outputs of every arm are compared: the fused call's files must inflate to the two calls' bytes.
One JSON line per measurement on stdout, and --readme (default profiles/fastq_prepare/README.md) is written from them: seconds, the bytes each
side read and wrote, the phases.  No ratio is fixed in advance; the yardstick is the two-call sequence on the same machine and files.
Usage: fastq_prepare_bench.py [--pairs 1000000] [--per-barcode 200] [--repeats 3] [--run-bytes 67108864] [--out-dir DIR] [--readme PATH]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bgzfio  # noqa: E402  (tests/bgzfio.py: the BGZF reader)
import fqsortcases as fc  # noqa: E402
from arachne_amd import api, synth  # noqa: E402
from fastq_standardize_bench import raw_tellseq, tell_code, write_bgzf  # noqa: E402  (the same input)

STD_PHASES = ("read", "inflate", "parse", "fields", "compose", "compress", "write")
SORT_PHASES = ("read", "inflate", "parse", "keys", "sort", "gather", "compress", "write", "run_write", "run_read")


def phases(st, names):
    return {p + "_ms": round(st[p + "_us"] / 1e3, 2) for p in names}


def text_of(path, bgzf):
    raw = open(path, "rb").read()
    return bgzfio.inflate(raw) if bgzf else raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--per-barcode", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--run-bytes", type=int, default=64 << 20)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--readme", default=os.path.join(ROOT, "profiles", "fastq_prepare", "README.md"))
    args = ap.parse_args()
    d = args.out_dir or tempfile.mkdtemp(prefix="arx_fqprep_bench_")
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
    raw_bytes = sum(len(t) for t in texts)
    del texts
    for p in plain + bz:                                         # into the page cache
        with open(p, "rb") as f:
            while f.read(1 << 24):
                pass
    rows = [dict(what="input", pairs=n, barcodes=len(codes), plain_bytes=sum(os.path.getsize(p) for p in plain), bgzf_bytes=sum(os.path.getsize(p) for p in bz), text_bytes=raw_bytes)]
    print(json.dumps(rows[0]), flush=True)
    tmp = os.path.join(d, "tmp")
    os.makedirs(tmp, exist_ok=True)
    summary = {}
    for form, src, bgzf in (("plain", plain, False), ("bgzf", bz, True)):
        for mode, rb in (("core", 0), ("runs", args.run_bytes)):
            arm = form + ", " + mode
            ext = ".gz" if bgzf else ""
            std = tuple(os.path.join(d, "std%d.fq%s" % (k, ext)) for k in (1, 2))
            two = tuple(os.path.join(d, "two%d.fq%s" % (k, ext)) for k in (1, 2))
            one = tuple(os.path.join(d, "one%d.fq%s" % (k, ext)) for k in (1, 2))
            series = dict(two_calls=[], prepare=[])
            for rep in range(args.repeats + 1):
                timed = rep == args.repeats
                t = time.time()
                a = api.fastq_standardize(*src, *std, format="auto", bgzf=bgzf, timed=timed)
                ta = time.time() - t
                b = api.fastq_sort_ex(*std, *two, bgzf=bgzf, timed=timed, run_bytes=rb, tmp_dir=tmp)
                s = time.time() - t
                between = sum(os.path.getsize(p) for p in std)
                row = dict(what="two_calls", arm=arm, timed=timed, seconds=round(s, 4), standardize_s=round(ta, 4), sort_s=round(s - ta, 4), pairs_per_s=round(n / s), records=b["records"],
                           text_read=a["bytes_in_r1"] + a["bytes_in_r2"] + b["bytes_in_r1"] + b["bytes_in_r2"],
                           text_written=a["bytes_out_r1"] + a["bytes_out_r2"] + b["bytes_out_r1"] + b["bytes_out_r2"] + b["tmp_bytes"], file_bytes_between=between,
                           file_bytes_out=sum(os.path.getsize(p) for p in two), sorted_runs=b["sorted_runs"], standardize=phases(a, STD_PHASES), sort=phases(b, SORT_PHASES))
                rows.append(row)
                print(json.dumps(row), flush=True)
                if not timed:
                    series["two_calls"].append(round(s, 4))
                t = time.time()
                c = api.fastq_prepare(*src, *one, format="auto", bgzf=bgzf, timed=timed, run_bytes=rb, tmp_dir=tmp)
                s = time.time() - t
                row = dict(what="prepare", arm=arm, timed=timed, seconds=round(s, 4), pairs_per_s=round(n / s), records=c["records"], format=c["format"],
                           text_read=c["bytes_in_r1"] + c["bytes_in_r2"], text_written=c["bytes_out_r1"] + c["bytes_out_r2"] + c["tmp_bytes"],
                           file_bytes_out=sum(os.path.getsize(p) for p in one), sorted_runs=c["sorted_runs"], prepare=phases(c, SORT_PHASES))
                if rep == 0:
                    row["output_is_the_two_calls"] = all(text_of(p, bgzf) == text_of(q, bgzf) for p, q in zip(one, two))
                    row["files_are_the_two_calls"] = all(open(p, "rb").read() == open(q, "rb").read() for p, q in zip(one, two))
                rows.append(row)
                print(json.dumps(row), flush=True)
                if not timed:
                    series["prepare"].append(round(s, 4))
            m2, m1 = statistics.median(series["two_calls"]), statistics.median(series["prepare"])
            summary[arm] = dict(two_calls_s=series["two_calls"], prepare_s=series["prepare"], two_calls_median_s=m2, prepare_median_s=m1, saved_s=round(m2 - m1, 4),
                                prepare_wins=m1 < m2)
    rows.append(dict(what="summary", **summary))
    print(json.dumps(rows[-1]), flush=True)
    write_readme(args, rows, summary)
    if not args.out_dir:
        shutil.rmtree(d, ignore_errors=True)


def write_readme(args, rows, summary):
    inp = rows[0]
    L = ["# profiles/fastq_prepare — standardize and sort in one call (`arx_fastq_prepare`) beside the two calls it replaces, MI355X", "",
         "Written by `tools/fastq_prepare_bench.py --pairs %d --per-barcode %d --repeats %d --run-bytes %d`." % (args.pairs, args.per_barcode, args.repeats, args.run_bytes), "",
         "Input: %d pairs of 2x150 bp in raw TELLseq form, %d barcodes; %d bytes of text, %d bytes as plain files, %d as BGZF; files in the page cache, outputs and"
         % (inp["pairs"], inp["barcodes"], inp["text_bytes"], inp["plain_bytes"], inp["bgzf_bytes"]),
         "temporary files on the machine's disk.  The yardstick is `arx_fastq_standardize` followed by `arx_fastq_sort_ex` on the same files in the same process,",
         "alternating with the fused call; the standardized files between the two calls are in the arm's form (plain or BGZF).  No ratio was fixed in advance.", "",
         "## Seconds per pair of files (untimed repeats; medians)", "",
         "| arm | two calls | `arx_fastq_prepare` | medians (two calls / prepare) | saved | the fused call wins |", "|---|---|---|---|---|---|"]
    for arm, s in summary.items():
        L.append("| %s | %s | %s | %.3f / %.3f | %.3f s | %s |" % (arm, ", ".join("%.3f" % x for x in s["two_calls_s"]), ", ".join("%.3f" % x for x in s["prepare_s"]),
                                                                   s["two_calls_median_s"], s["prepare_median_s"], s["saved_s"], "yes" if s["prepare_wins"] else "NO"))
    L += ["", "## Bytes (first repeat of each arm)", "",
          "| arm | side | inflated text read | inflated text written (outputs and run files) | file bytes between the calls | file bytes out | sorted runs | equal to the two calls |",
          "|---|---|---|---|---|---|---|---|"]
    seen = set()
    for r in rows[1:-1]:
        if r["timed"] or (r["arm"], r["what"]) in seen:
            continue
        seen.add((r["arm"], r["what"]))
        eq = "" if r["what"] == "two_calls" else "text %s, files %s" % (r.get("output_is_the_two_calls"), r.get("files_are_the_two_calls"))
        L.append("| %s | %s | %d | %d | %s | %d | %d | %s |" % (r["arm"], r["what"], r["text_read"], r["text_written"], r.get("file_bytes_between", "—"), r["file_bytes_out"], r["sorted_runs"], eq))
    L += ["", "## Phases, milliseconds (the TIMED pass: every launch group awaited, so the sums exceed an untimed call)", "", "| arm | call | seconds | " + " | ".join(SORT_PHASES) + " |",
          "|---|---|---|" + "---|" * len(SORT_PHASES)]
    for r in rows[1:-1]:
        if not r["timed"]:
            continue
        if r["what"] == "two_calls":
            a, b = r["standardize"], r["sort"]
            L.append("| %s | standardize | %.3f | " % (r["arm"], r["standardize_s"]) + " | ".join(str(a.get(p + "_ms", a.get({"keys": "fields", "gather": "compose"}.get(p, p) + "_ms", "—"))) for p in SORT_PHASES) + " |")
            L.append("| %s | sort_ex | %.3f | " % (r["arm"], r["sort_s"]) + " | ".join(str(b[p + "_ms"]) for p in SORT_PHASES) + " |")
        else:
            L.append("| %s | prepare | %.3f | " % (r["arm"], r["seconds"]) + " | ".join(str(r["prepare"][p + "_ms"]) for p in SORT_PHASES) + " |")
    L += ["", "(standardize's `fields` stands under keys and its `compose` under gather.)", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.readme)), exist_ok=True)
    with open(args.readme, "w") as f:
        f.write("\n".join(L))


if __name__ == "__main__":
    main()

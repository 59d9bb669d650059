#!/usr/bin/env python3
"""The .bai or the .csi of a coordinate-sorted BAM file on the GPU (arx_bam_index, arx_bam_index_csi), phase by phase, next to the sort that
made the file.

The bucket of tools/bam_sort_bench.py (--records typical 2x150 bp records on random positions of one contig, written by the host sink) is
sorted into one file by arx_bam_sort_append (host writer), and that file is indexed.  One JSON line per measurement:
  append   arx_bam_sort_append of the bucket into the host writer: the seconds of the call and of the close that follows
  index    arx_bam_index of the sorted file, plain and with ARX_BAI_TIMED (which waits for every launch): the phases in ms, the counts
           of runs, chunks, bins and linear entries, and max_bytes (0: the 256 MiB default; --slab sets a second size).  --format csi:
           arx_bam_index_csi of the same file at min_shift 14 (the BAI's scheme on these contigs): depth in place of the linear entries
  arm      --arms: the index as a second pass against the index in the writer, on the same build and bucket, for both sinks, the two arms
           alternating, pass 0 of each not counted.  Arm A: arx_bam_sort_append into a plain writer, the close, then arx_bam_index of the
           file.  Arm B: the same append into the indexing writer (api.BamWriter(index=...)) and its close, which writes the index.  A last
           line (what: verdict) holds, per sink, B's median of append + close against A's fastest append + close + index, and against A's
           append + close alone -- what the index costs now.  The two indexes must be the same bytes
Usage: bam_index_bench.py [--records 2000000] [--repeats 3] [--slab 33554432] [--format bai|csi] [--arms]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from arachne_amd import api, synth
from bam_sort_bench import make_bucket

PHASES = ("read", "inflate", "discover", "records", "runs", "write", "total")


def arms(args, ref, bucket, d):
    """the second pass (A) against the index in the writer (B), alternating, for both sinks"""
    names, offs, clens, alt, l_pac = ref.contigs()
    index_file = api.bam_index_csi if args.format == "csi" else api.bam_index
    verdict = {}
    for sink in ("host", "device"):
        took = dict(A=[], A_bam=[], B=[])
        for rep in range(args.repeats + 1):
            for arm in ("A", "B"):
                final = os.path.join(d, "arm_%s_%s.bam" % (arm, sink))
                for leftover in (final + "." + args.format,):
                    if os.path.exists(leftover):
                        os.remove(leftover)
                kw = dict(index=args.format, index_device=ref) if arm == "B" else dict(coordinate=True)
                w = api.BamWriter(final, names, clens, extra_header="@PG\tID:bench\n", threads=16, level=1, device=ref if sink == "device" else None, **kw)
                t = time.time()
                st = w.sort_append(ref, bucket)
                t_append = time.time() - t
                t = time.time()
                closed = w.close()
                t_close = time.time() - t
                t_index, ist = 0.0, closed.get("index")
                if arm == "A":
                    t = time.time()
                    ist = index_file(final, device=ref.device)
                    t_index = time.time() - t
                assert st["records"] == ist["records"] == args.records
                if rep > 0:
                    took[arm].append(t_append + t_close + t_index)
                    if arm == "A":
                        took["A_bam"].append(t_append + t_close)
                print(json.dumps(dict(what="arm", arm=arm, sink=sink, format=args.format, counted=rep > 0, append_seconds=round(t_append, 4), close_seconds=round(t_close, 4),
                                      index_seconds=round(t_index, 4), seconds=round(t_append + t_close + t_index, 4), file_bytes=closed["bytes_out"],
                                      indexing_ms=round(ist["total_us"] / 1e3, 3), slabs=ist["slabs"], runs=ist["runs"], chunks=ist["chunks"])), flush=True)
            a, b = (open(os.path.join(d, "arm_%s_%s.bam" % (x, sink)), "rb").read() for x in "AB")
            ia, ib = (open(os.path.join(d, "arm_%s_%s.bam.%s" % (x, sink, args.format)), "rb").read() for x in "AB")
            assert a == b and ia == ib, "the arms disagree"
        med = lambda v: sorted(v)[len(v) // 2]
        verdict[sink] = dict(B_median=round(med(took["B"]), 4), A_fastest=round(min(took["A"]), 4), A_bam_only_median=round(med(took["A_bam"]), 4),
                             index_cost=round(med(took["B"]) - med(took["A_bam"]), 4), passes=len(took["B"]), holds=med(took["B"]) < min(took["A"]))
    print(json.dumps(dict(what="verdict", criterion="B's median of append + close below A's fastest append + close + index", **verdict)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slab", type=int, default=32 << 20)
    ap.add_argument("--format", choices=("bai", "csi"), default="bai")
    ap.add_argument("--arms", action="store_true")
    args = ap.parse_args()
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    d = tempfile.mkdtemp(prefix="arx_index_bench_", dir=tmp)
    try:
        g = synth.make_genome(15, [400000, 150000])
        fa = os.path.join(d, "g.fa")
        g.write_fasta(fa)
        api.index_build(fa, fa)
        ref = api.Reference(fa)
        names, offs, clens, alt, l_pac = ref.contigs()
        bucket, final = os.path.join(d, "bucket.bam"), os.path.join(d, "sorted.bam")
        made = make_bucket(bucket, ref, args.records)
        print(json.dumps(dict(what="input", records=made["records"], file_bytes=made["bytes_out"])), flush=True)
        if args.arms:
            arms(args, ref, bucket, d)
            ref.close()
            return
        for rep in range(args.repeats + 1):                     # pass 0 is not counted: code objects, rocprim's first calls
            w = api.BamWriter(final, names, clens, extra_header="@PG\tID:bench\n", threads=16, level=1, coordinate=True)
            t = time.time()
            st = w.sort_append(ref, bucket)
            dt = time.time() - t
            t = time.time()
            closed = w.close()
            print(json.dumps(dict(what="append", counted=rep > 0, seconds=round(dt, 4), close_seconds=round(time.time() - t, 4), file_bytes=closed["bytes_out"],
                                  inflated_bytes=st["inflated_bytes"])), flush=True)
        for rep in range(args.repeats + 1):
            for max_bytes in (0, args.slab):
                for timed in (False, True):
                    t = time.time()
                    st = (api.bam_index_csi if args.format == "csi" else api.bam_index)(final, max_bytes=max_bytes, timed=timed, device=ref.device)
                    dt = time.time() - t
                    assert st["records"] == args.records
                    own = dict(depth=st["depth"], min_shift=st["min_shift"], csi_bytes=os.path.getsize(final + ".csi")) if args.format == "csi" else \
                        dict(linear=st["linear"], bai_bytes=os.path.getsize(final + ".bai"))
                    print(json.dumps(dict(what="index", format=args.format, counted=rep > 0, max_bytes=max_bytes, timed=timed, seconds=round(dt, 4), slabs=st["slabs"],
                                          blocks=st["blocks"], runs=st["runs"], chunks=st["chunks"], bins=st["bins"], **own,
                                          ms={p: round(st[p + "_us"] / 1e3, 3) for p in PHASES})), flush=True)
        ref.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The FASTQ feeders alone and one-pair end to end, on the GPU box: the read set of a bench.py workload (default: the 1 M-pair TELLseq-like
set of the headline command, genome and index from bench.py's cache) written with synth.write_fastq_fast as ONE plain pair and ONE gzip pair,
files in the page cache.  --bgzf adds ONE BGZF pair (blocks of 65,280 bytes at level 4: what `samtools fastq -c 4` writes) and, with
--inflate device (or both), the device feeder with the inflate on the GPU (arx_feeder_open_device_ex) as a third arm on it.

  feeder alone   arx_feeder_next until the end of the input, pairs/s: the host feeder (arx_feeder_open) against the device feeder
                 (arx_feeder_open_device, depth 1: the host feeder's contract), --repeats runs each, alternating, plain and gzip
  end to end     e2e.run on that one pair: the host feeder with its one worker against feeder="device" with --workers workers

One JSON line per measurement on stdout, a table on stderr.  Usage: feeder_bench.py [--workload grch38] [--repeats 5] [--workers 3]
[--chunk-bytes 0] [--pairs-per-batch 250000] [--no-e2e] [--bgzf] [--inflate host|device|both] [--e2e-passes 3] [--out-dir DIR]"""
import argparse
import gzip
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402  (the workloads, the cached genome and index)
import bgzfio  # noqa: E402  (tests/bgzfio.py: the BGZF writer)
from arachne_amd import api, e2e, synth  # noqa: E402


def feed(make, target):
    """-> (pairs, super-batches, seconds) of one pass over the input"""
    t = time.time()
    fd = make()
    pairs = n = 0
    while True:
        nx = fd.next_raw(target)
        if nx is None:
            break
        pairs += int(nx[1]["n_pairs"]); n += 1
    st = fd.stats() if fd.device is not None else None
    fd.close()
    return pairs, n, time.time() - t, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="grch38", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workers", type=int, default=3)
    ap.add_argument("--chunk-bytes", type=int, default=0)
    ap.add_argument("--pairs-per-batch", type=int, default=250_000)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--e2e-passes", type=int, default=3, help="end-to-end passes per arm, the arms alternating")
    ap.add_argument("--bgzf", action="store_true", help="also write the input as one BGZF pair and run the feeders on it")
    ap.add_argument("--inflate", default="host", choices=["host", "device", "both"], help="where the device feeder inflates BGZF input (both: an arm each)")
    ap.add_argument("--cache", default="/tmp/arx_bench_cache")
    ap.add_argument("--lib", default=api.LIB_PATH, help="(dry runs of this script only) alternative library exporting the C ABI")
    ap.add_argument("--out-dir", default=None, help="where the FASTQ and BAM files go (default: <cache>/feeder_bench_<pid>; removed afterwards)")
    args = ap.parse_args()
    wl = bench.WORKLOADS[args.workload]
    lib = api.LIB_PATH = args.lib
    prefix = bench.prepare_index(args.cache, args.workload, wl["lens"], wl["seed"], wl["families"], 0, lambda: None, {}, alt_spec=wl.get("alt_spec"),
                                 decoy_spec=wl.get("decoy_spec"))
    rs = bench.workload_reads(wl, wl["seed"] + 1000, bench.load_genome(prefix), wl["barcodes"], wl["ppb"])
    d = args.out_dir or os.path.join(args.cache, "feeder_bench_%d" % os.getpid())
    os.makedirs(d, exist_ok=True)
    plain = (os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq"))
    synth.write_fastq_fast(rs, *plain)
    gz = tuple(p + ".gz" for p in plain)
    for p, q in zip(plain, gz):
        with open(p, "rb") as f, gzip.open(q, "wb", compresslevel=1) as g:
            shutil.copyfileobj(f, g, 1 << 24)
    bz = tuple(p + ".bgzf.gz" for p in plain) if args.bgzf else ()
    for p, q in zip(plain, bz):
        with open(p, "rb") as f, open(q, "wb") as g:
            while True:
                part = f.read(256 * bgzfio.BLOCK_IN)
                if not part:
                    break
                g.write(bgzfio.write_bgzf(part, level=4, eof=False))
            g.write(bgzfio.EOF_BLOCK)
    for p in plain + gz + bz:                    # into the page cache
        with open(p, "rb") as f:
            while f.read(1 << 24):
                pass
    sizes = dict(pairs=rs.n_pairs, plain_bytes=sum(os.path.getsize(p) for p in plain), gzip_bytes=sum(os.path.getsize(p) for p in gz),
                 bgzf_bytes=sum(os.path.getsize(p) for p in bz))
    print(json.dumps(dict(what="input", workload=args.workload, **sizes)), flush=True)
    ref = api.Reference(prefix, lib_path=lib)
    rows = []
    try:
        dev_arms = {"host": ["device"], "device": ["device, inflate on the device"], "both": ["device", "device, inflate on the device"]}[args.inflate]
        for kind, files in (("plain", plain), ("gzip", gz)) + ((("bgzf", bz),) if bz else ()):
            arms = ["host"] + (dev_arms if kind == "bgzf" else ["device"])
            res = {who: [] for who in arms}

            def maker(who):
                if who == "host":
                    return lambda: api.Feeder(*files, lib_path=lib)
                return lambda: api.Feeder(*files, lib_path=lib, device=ref, chunk_bytes=args.chunk_bytes, depth=1, inflate="device" if "inflate" in who else "host")
            feed(maker(arms[-1]), args.pairs_per_batch)   # warm-up: code objects, page-locked buffers
            for _ in range(args.repeats):
                for who in arms:
                    make = maker(who)
                    pairs, n, s, st = feed(make, args.pairs_per_batch)
                    assert pairs == rs.n_pairs, (pairs, rs.n_pairs)
                    res[who].append(pairs / s)
                    print(json.dumps(dict(what="feeder", input=kind, feeder=who, pairs=pairs, super_batches=n, seconds=round(s, 4), pairs_per_s=round(pairs / s), stats=st)), flush=True)
            for who in arms:
                v = sorted(res[who])
                rows.append((f"feeder alone, {kind}", who, v[len(v) // 2], v[0], v[-1]))
        if not args.no_e2e:
            kw = dict(pairs_per_batch=args.pairs_per_batch, bam_threads=8, rec_threads=8, lib_path=lib)
            for who in ("host", "device") * args.e2e_passes:      # the first two passes also pay for the handles' work memory
                out = os.path.join(d, "out_" + who)
                st = e2e.run(ref, [plain], out, **kw) if who == "host" else e2e.run(ref, [plain], out, feeder="device", workers=args.workers, chunk_bytes=args.chunk_bytes, **kw)
                assert st["pairs"] == rs.n_pairs
                print(json.dumps(dict(what="e2e", feeder=who, workers=st["workers"], pairs=st["pairs"], seconds=round(st["seconds"], 4), pairs_per_s=round(st["pairs_per_s"]),
                                      worker_seconds={k: round(st[k], 3) for k in ("feeder_s", "device_s", "fetch_s", "records_s", "bam_s")})), flush=True)
                rows.append(("end to end, plain, one pair", who + (" (1 worker)" if who == "host" else f" ({args.workers} workers)"), st["pairs_per_s"], st["pairs_per_s"], st["pairs_per_s"]))
            for inflate in ([] if not bz else ["host", "device"] * args.e2e_passes if args.inflate == "both" else [args.inflate] * args.e2e_passes):
                st = e2e.run(ref, [bz], os.path.join(d, "out_bgzf_" + inflate), feeder="device", workers=args.workers, chunk_bytes=args.chunk_bytes, inflate=inflate, **kw)
                assert st["pairs"] == rs.n_pairs
                print(json.dumps(dict(what="e2e", input="bgzf", feeder="device", inflate=inflate, workers=st["workers"], pairs=st["pairs"], seconds=round(st["seconds"], 4),
                                      pairs_per_s=round(st["pairs_per_s"]), feeder_stats=st.get("feeder"))), flush=True)
                rows.append(("end to end, bgzf, one pair", f"device, inflate {inflate} ({args.workers} workers)", st["pairs_per_s"], st["pairs_per_s"], st["pairs_per_s"]))
    finally:
        ref.close()
        if not args.out_dir:
            shutil.rmtree(d, ignore_errors=True)
    merged = {}
    for what, who, mid, lo, hi in rows:                       # the end-to-end passes of an arm: one row with their range
        merged.setdefault((what, who), []).extend([mid] if lo == hi == mid else [lo, mid, hi])
    rows = [(what, who, sorted(v)[len(v) // 2], min(v), max(v)) for (what, who), v in merged.items()]
    for what, who, mid, lo, hi in rows:
        print(f"{what:32s} {who:22s} {mid / 1e6:6.3f} M pairs/s  (min {lo / 1e6:.3f}, max {hi / 1e6:.3f})", file=sys.stderr)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The device feeder on ordinary gzip input: the inflate on the GPU (gunzip="device": ARX_FEEDER_GUNZIP_DEVICE, both files' launches in flight at
once) against zlib on the two reader threads (gunzip="host", which is what the feeder did before the flag existed).  The read set is the 1 M-pair
set of tools/feeder_bench.py (a bench.py workload, genome and index from bench.py's cache), written as ONE gzip pair at level 1 and ONE at
level 6, files in the page cache.

  feeder   the device feeder alone (depth 1), arx_feeder_next until the end of the input: the two arms alternate, --repeats passes each, per level
  e2e      e2e.run(feeder="device", workers=--workers) on the level-1 pair, the two arms alternating, --e2e-passes passes each
  find     arx_selftest_gunzip on R1 of the level-1 pair at 32 KiB chunks, --repeats times: seconds and the phase times (find, decode, windows +
           resolve); with --parent-lib PATH the same on another build's library, the two builds alternating

One JSON line per pass on stdout, a table on stderr.  Usage: feeder_gunzip_bench.py [--steps feeder,e2e,find] [--workload grch38] [--repeats 3]
[--e2e-passes 3] [--e2e-warm 2] [--parent-lib PATH] [--workers 3] [--chunk-bytes 0] [--pairs-per-batch 250000] [--lib PATH] [--out-dir DIR]"""
import argparse
import gzip
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workloads, the cached genome and index)
from arachne_amd import api, e2e, synth  # noqa: E402


def feed(ref, files, gunzip, chunk_bytes, target, lib):
    """-> (pairs, super-batches, seconds, the feeder's stats, the two files' gunzip stats) of one pass over the input"""
    t = time.time()
    fd = api.Feeder(*files, lib_path=lib, device=ref, chunk_bytes=chunk_bytes, depth=1, gunzip=gunzip)
    pairs = n = 0
    while True:
        nx = fd.next_raw(target)
        if nx is None:
            break
        pairs += int(nx[1]["n_pairs"]); n += 1
    st, gs = fd.stats(), fd.gunzip_stats()
    fd.close()
    return pairs, n, time.time() - t, st, gs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="feeder,e2e,find")
    ap.add_argument("--workload", default="grch38", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--e2e-passes", type=int, default=3)
    ap.add_argument("--e2e-warm", type=int, default=2, help="untimed end-to-end passes per arm first")
    ap.add_argument("--workers", type=int, default=3)
    ap.add_argument("--chunk-bytes", type=int, default=0)
    ap.add_argument("--pairs-per-batch", type=int, default=250_000)
    ap.add_argument("--cache", default="/tmp/arx_bench_cache")
    ap.add_argument("--lib", default=api.LIB_PATH, help="alternative library exporting the C ABI (the find step on another build)")
    ap.add_argument("--parent-lib", default=None, help="the find step also on this library (the parent commit's build), the two alternating")
    ap.add_argument("--out-dir", default=None, help="where the FASTQ and BAM files go (default: <cache>/feeder_gunzip_bench_<pid>; removed afterwards)")
    args = ap.parse_args()
    steps = set(args.steps.split(","))
    assert steps <= {"feeder", "e2e", "find"} and args.repeats >= 1, args.steps
    wl = bench.WORKLOADS[args.workload]
    lib = api.LIB_PATH = args.lib
    prefix = bench.prepare_index(args.cache, args.workload, wl["lens"], wl["seed"], wl["families"], 0, lambda: None, {}, alt_spec=wl.get("alt_spec"),
                                 decoy_spec=wl.get("decoy_spec"))
    rs = bench.workload_reads(wl, wl["seed"] + 1000, bench.load_genome(prefix), wl["barcodes"], wl["ppb"])
    d = args.out_dir or os.path.join(args.cache, "feeder_gunzip_bench_%d" % os.getpid())
    os.makedirs(d, exist_ok=True)
    plain = (os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq"))
    synth.write_fastq_fast(rs, *plain)
    pair = {}
    for level in (1, 6) if "feeder" in steps else (1,):
        pair[level] = tuple("%s.l%d.gz" % (p, level) for p in plain)
        for p, q in zip(plain, pair[level]):
            with open(p, "rb") as f, gzip.open(q, "wb", compresslevel=level) as g:
                shutil.copyfileobj(f, g, 1 << 24)
            with open(q, "rb") as f:             # into the page cache
                while f.read(1 << 24):
                    pass
    print(json.dumps(dict(what="input", workload=args.workload, pairs=rs.n_pairs, plain_bytes=sum(os.path.getsize(p) for p in plain),
                          gzip_bytes={level: sum(os.path.getsize(p) for p in ps) for level, ps in pair.items()})), flush=True)
    rows = {}
    ref = api.Reference(prefix, lib_path=lib) if steps & {"feeder", "e2e"} else None
    try:
        if "feeder" in steps:
            for level, files in pair.items():
                feed(ref, files, "device", args.chunk_bytes, args.pairs_per_batch, lib)          # warm-up: code objects, page-locked buffers
                for _ in range(args.repeats):
                    for gunzip in ("host", "device"):
                        pairs, n, s, st, gs = feed(ref, files, gunzip, args.chunk_bytes, args.pairs_per_batch, lib)
                        assert pairs == rs.n_pairs, (pairs, rs.n_pairs)
                        rows.setdefault(("feeder alone, gzip level %d" % level, "gunzip=" + gunzip), []).append(pairs / s)
                        print(json.dumps(dict(what="feeder", level=level, gunzip=gunzip, pairs=pairs, super_batches=n, seconds=round(s, 4), pairs_per_s=round(pairs / s), stats=st,
                                              gunzip_stats=gs if gunzip == "device" else None)), flush=True)
        if "e2e" in steps:
            kw = dict(pairs_per_batch=args.pairs_per_batch, bam_threads=8, rec_threads=8, lib_path=lib, feeder="device", workers=args.workers, chunk_bytes=args.chunk_bytes)
            for k, gunzip in enumerate(("host", "device") * (args.e2e_warm + args.e2e_passes)):
                st = e2e.run(ref, [pair[1]], os.path.join(d, "out_" + gunzip), gunzip=gunzip, **kw)
                assert st["pairs"] == rs.n_pairs
                if k < 2 * args.e2e_warm:                             # warm-up passes of both arms: the handles' work memory, the code objects
                    continue
                rows.setdefault(("end to end, gzip level 1, %d workers" % args.workers, "gunzip=" + gunzip), []).append(st["pairs_per_s"])
                print(json.dumps(dict(what="e2e", gunzip=gunzip, workers=st["workers"], pairs=st["pairs"], seconds=round(st["seconds"], 4), pairs_per_s=round(st["pairs_per_s"]),
                                      worker_seconds={k: round(st[k], 3) for k in ("feeder_s", "device_s", "fetch_s", "records_s", "bam_s")}, gunzip_stats=st.get("gunzip"))), flush=True)
        if "find" in steps:
            data = open(pair[1][0], "rb").read()
            builds = [("this", lib)] + ([("parent", args.parent_lib)] if args.parent_lib else [])
            for k in range(args.repeats + 1):                         # (the first run of each pays for the code objects and is not reported)
                for build, path in builds:                            # the builds alternate
                    t = time.time()
                    r = api.selftest_gunzip(data, chunk_bytes=32 << 10, cap=os.path.getsize(plain[0]) + 64, lib_path=path)
                    s = time.time() - t
                    assert r["rc"] == 0 and len(r["out"]) == os.path.getsize(plain[0])
                    if k:
                        rows.setdefault(("arx_selftest_gunzip, R1 level 1", "%s: find, us" % build), []).append(r["us_find"])
                        print(json.dumps(dict(what="find", build=build, seconds=round(s, 4), **{x: r[x] for x in api.GUNZIP_STATS})), flush=True)
    finally:
        if ref is not None:
            ref.close()
        if not args.out_dir:
            shutil.rmtree(d, ignore_errors=True)
    for (what, who), v in rows.items():
        v = sorted(v)
        unit = (1.0, "us") if who.endswith("us") else (1e6, "M pairs/s")
        print(f"{what:40s} {who:16s} {v[len(v) // 2] / unit[0]:10.3f} {unit[1]}  (min {v[0] / unit[0]:.3f}, max {v[-1] / unit[0]:.3f})", file=sys.stderr)


if __name__ == "__main__":
    main()

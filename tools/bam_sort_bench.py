#!/usr/bin/env python3
"""The coordinate sort of one position bucket on the GPU (arx_bam_sort_append, arx_selftest_bam_sort), phase by phase.

A synthetic bucket of --records typical 2x150 bp records (name, one CIGAR op, 150 bases + qualities, ~45 bytes of aux) on random positions of
one contig, written by the host sink.  One JSON line per measurement:
  sort      the kernels alone on the inflated record bytes (arx_selftest_bam_sort, ARX_SORT_TIMED) at every --seg: probe, walk, repair, keys,
            sort, gather in ms and GB/s of inflated bytes, and the segments repaired
  host      the yardstick: tests/sortsim/bam_sort_sim.cpp, built here without the sanitizers, std::stable_sort, one thread, the same bytes
  append    arx_bam_sort_append of the file into a host and into a device writer (the library's seg_bytes): read, inflate, the kernel phases,
            compress and write
  finalize  (--e2e WORKLOAD) e2e.run(layout="reference", feeder="device") over the workload's read set, then e2e.finalize over its
            directory with each sink, next to the pass's own seconds
Usage: bam_sort_bench.py [--records 2000000] [--seg 262144 1048576 4194304] [--repeats 3] [--e2e grch38] [--cache DIR]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from arachne_amd import api, e2e, synth

PHASES = ("read", "inflate", "probe", "walk", "repair", "keys", "sort", "gather", "write", "total")


def phases(st, n_bytes):
    out = {}
    for p in PHASES:
        us = st[p + "_us"]
        out[p] = dict(ms=round(us / 1e3, 3), GB_per_s=round(n_bytes / us / 1e3, 2) if us else None)
    return out


def make_bucket(path, ref, n, threads=16):
    names, offs, clens, alt, l_pac = ref.contigs()
    rng = np.random.default_rng(1)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, 150), dtype=np.uint8)]
    qual = (rng.integers(2, 41, size=(n, 150), dtype=np.uint8) + 33).astype(np.uint8)
    aux1 = b"RGZlib1\0ASC\x96XMZ0\0AMZ1\0XTC\0BXZA01C02B03D04-1\0VXC\x01"
    name_b = np.frombuffer(b"".join(b"r%09d" % i for i in range(n)), dtype=np.uint8)
    name_off = np.arange(n + 1, dtype=np.int64) * 10
    flag = np.full(n, 99, np.int32); rid = np.zeros(n, np.int32); pos = rng.integers(0, int(clens[0]) - 200, size=n).astype(np.int32); mapq = np.full(n, 60, np.uint8)
    mpos = pos + 200; tlen = np.full(n, 350, np.int32)
    cig_off = np.arange(n + 1, dtype=np.int64); cig = np.full(n, 150 << 4, np.uint32)
    seq_off = np.arange(n + 1, dtype=np.int64) * 150
    aux_off = np.arange(n + 1, dtype=np.int64) * len(aux1); aux_b = np.frombuffer(aux1 * n, dtype=np.uint8)
    b = api._BamBatch(n, name_off.ctypes.data, name_b.ctypes.data, flag.ctypes.data, rid.ctypes.data, pos.ctypes.data, mapq.ctypes.data, rid.ctypes.data, mpos.ctypes.data,
                      tlen.ctypes.data, cig_off.ctypes.data, cig.ctypes.data, seq_off.ctypes.data, seq.ctypes.data, qual.ctypes.data, 33, aux_off.ctypes.data, aux_b.ctypes.data)
    w = api.BamWriter(path, names, clens, extra_header="@PG\tID:bench\n", threads=threads, level=1)
    w.write_view(b)
    return w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--seg", type=int, nargs="*", default=[1 << 18, 1 << 20, 1 << 22])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--e2e", default=None, help="a bench.py workload: run the reference layout over its read set and finalize its directory")
    ap.add_argument("--cache", default="/tmp/arx_bench_cache")
    ap.add_argument("--pairs-per-batch", type=int, default=250_000)
    ap.add_argument("--workers", type=int, default=3)
    args = ap.parse_args()
    import reccases as rc
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    d = tempfile.mkdtemp(prefix="arx_sort_bench_", dir=tmp)
    try:
        g = synth.make_genome(15, [400000, 150000])
        fa = os.path.join(d, "g.fa")
        g.write_fasta(fa)
        api.index_build(fa, fa)
        ref = api.Reference(fa)
        names, offs, clens, alt, l_pac = ref.contigs()
        bucket = os.path.join(d, "bucket.bam")
        t = time.time()
        made = make_bucket(bucket, ref, args.records)
        data = rc.inflate(bucket)
        stream = data[rc.header_len(data):]
        del data
        print(json.dumps(dict(what="input", records=made["records"], inflated_bytes=len(stream), file_bytes=made["bytes_out"], seconds_to_make=round(time.time() - t, 1))), flush=True)
        # ---- the kernels alone
        for rep in range(args.repeats + 1):                     # pass 0 is not counted: code objects, rocprim's first calls
            for seg in args.seg:
                r = api.selftest_bam_sort(stream, len(names), seg, timed=True)
                assert r["rc"] == 0 and r["n_records"] == args.records
                st = r["stats"]
                print(json.dumps(dict(what="sort", counted=rep > 0, seg_bytes=seg, segments=st["segments"], guess_right=st["guess_right"], repaired=st["repaired"],
                                      rounds=st["rounds"], phases={k: v for k, v in phases(st, len(stream)).items() if k not in ("read", "inflate", "write")})), flush=True)
        keys = np.array([(int.from_bytes(r["out"][o + 4:o + 8], "little") << 32) | int.from_bytes(r["out"][o + 8:o + 12], "little") for o in r["rec_off"][:args.records:997].tolist()])
        assert (np.diff(keys) >= 0).all()
        del r
        # ---- the host yardstick
        raw = os.path.join(d, "records.bin")
        with open(raw, "wb") as f:
            f.write(stream)
        exe_dir = tempfile.mkdtemp(prefix="arx_sort_sim_")        # (not next to the data: /dev/shm is often mounted noexec)
        exe = os.path.join(exe_dir, "bam_sort_sim")
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "sortsim", "bam_sort_sim.cpp"), "-o", exe])
        for rep in range(args.repeats):
            o = subprocess.run([exe, "time", raw, str(len(names)), str(1 << 20)], capture_output=True, text=True, check=True).stdout.split()
            ms = float(o[o.index("ms") + 1])
            print(json.dumps(dict(what="host", records=int(o[o.index("records") + 1]), ms=ms, GB_per_s=round(len(stream) / ms / 1e6, 3))), flush=True)
        os.remove(raw)
        shutil.rmtree(exe_dir, ignore_errors=True)
        # ---- into a writer
        for rep in range(args.repeats + 1):
            for sink in ("host", "device"):
                out = os.path.join(d, "sorted_%s.bam" % sink)
                w = api.BamWriter(out, names, clens, extra_header="@PG\tID:bench\n", threads=16, level=1, device=ref if sink == "device" else None, coordinate=True)
                t = time.time()
                st = w.sort_append(ref, bucket, timed=True)
                dt = time.time() - t
                t = time.time()
                closed = w.close()
                assert closed["records"] == args.records
                print(json.dumps(dict(what="append", counted=rep > 0, sink=sink, seconds=round(dt, 4), close_seconds=round(time.time() - t, 4), file_bytes=closed["bytes_out"],
                                      repaired=st["repaired"], segments=st["segments"], phases=phases(st, st["inflated_bytes"]))), flush=True)
        ref.close()
        # ---- a run's directory
        if args.e2e:
            import bench
            wl = bench.WORKLOADS[args.e2e]
            prefix = bench.prepare_index(args.cache, args.e2e, wl["lens"], wl["seed"], wl["families"], 0, lambda: None, {}, alt_spec=wl.get("alt_spec"),
                                         decoy_spec=wl.get("decoy_spec"))
            rs = bench.workload_reads(wl, wl["seed"] + 1000, bench.load_genome(prefix), wl["barcodes"], wl["ppb"])
            plain = (os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq"))
            synth.write_fastq_fast(rs, *plain)
            ref = api.Reference(prefix)
            out = os.path.join(d, "out")
            for rep in range(args.repeats):
                st = e2e.run(ref, [plain], out, pairs_per_batch=args.pairs_per_batch, bam_threads=8, rec_threads=8, layout="reference", feeder="device", workers=args.workers)
                print(json.dumps(dict(what="e2e", counted=rep > 0, pairs=st["pairs"], records=st["records"], seconds=round(st["seconds"], 3), files=len(st["files"]))), flush=True)
                for sink in ("host", "device"):
                    fin = e2e.finalize(ref, out, os.path.join(d, "final.bam"), sink=sink)
                    per = fin.pop("sort")
                    big = max(per, key=lambda x: x["records"])
                    print(json.dumps(dict(what="finalize", counted=rep > 0, sink=sink, seconds=round(fin["seconds"], 3), records=fin["records"], buckets=fin["buckets"],
                                          bytes=fin["bytes"], repaired=sum(x["repaired"] for x in per), segments=sum(x["segments"] for x in per),
                                          largest_bucket=dict(file=big["file"], records=big["records"], inflated_bytes=big["inflated_bytes"], ms=round(big["total_us"] / 1e3, 1)))), flush=True)
            ref.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

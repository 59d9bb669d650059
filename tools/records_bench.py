#!/usr/bin/env python3
"""The records phase (arx_batch_records) measured on the GPU box, on the read set of a bench.py workload (default: the 1 M-pair TELLseq-like set
of the headline command at the default step size, genome and index from bench.py's cache) written as ONE plain FASTQ pair, files in the page cache.

  kernels     the whole read set as one batch: run, rfa, post once, then arx_batch_records --repeats times with the kernel timers on -> ms per
              call of rec_size / scan / rec_tile / rec_fill; the fill's compulsory bytes (read: bases, qualities, names, read groups, CIGAR
              words, RecMeta, offsets; written: the stream) over its time as a fraction of --hbm-peak
  pcie        per 1 M pairs, from the batch's own counts: bytes each way for records="host" (slabs home; with the device sink the encoded
              stream up again) against records="device" (the super-batch's qualities / names / tables up; the stream home, or nothing)
  e2e         e2e.run on that pair, four arms records x sink, alternating, --repeats passes each after one untimed pass per arm

--layout reference adds the full records phase (arx_batch_records_full) and measures the reference's layout instead of the workers':
  kernels     arx_batch_tags once, then arx_batch_records_full --repeats times -> ms per call of its launches (rec_mm_len, rec_full_count,
              rec_full_meta, rec_tile and rec_full_fill -- two calls each per phase: the stream and the grouped stream --, the rec_group_* launches,
              scan), its stream bytes
  pcie        records="host" brings the slabs, the post phase's records, the mismatch lists and the tags home and, with the device sink, sends
              every record up twice; records="device_full" sends the super-batch's arrays up and brings both streams home, or nothing
  e2e         e2e.run(layout="reference") with records="host" (the baseline: the parent's path) against records="device_full", both sinks,
              alternating

One JSON line per measurement on stdout, a table on stderr.  Usage: records_bench.py [--workload grch38] [--repeats 5] [--feeder device]
[--workers 3] [--pairs-per-batch 250000] [--layout workers|reference] [--chunk 40000000] [--no-e2e] [--out-dir DIR]"""
import argparse
import json
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workloads, the cached genome and index)
from arachne_amd import api, e2e, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="grch38", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--barcodes", type=int, default=0, help="override the workload's barcodes")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--feeder", default="device", choices=["host", "device"])
    ap.add_argument("--workers", type=int, default=3)
    ap.add_argument("--pairs-per-batch", type=int, default=250_000)
    ap.add_argument("--hbm-peak", type=float, default=8e12, help="bytes/s the fill's traffic is set against")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--layout", default="workers", choices=["workers", "reference"], help="reference: also the full records phase, and the e2e arms of the reference's layout")
    ap.add_argument("--chunk", type=int, default=40_000_000, help="bases per position bucket (--layout reference)")
    ap.add_argument("--cache", default="/tmp/arx_bench_cache")
    ap.add_argument("--lib", default=api.LIB_PATH, help="(dry runs of this script only) alternative library exporting the C ABI")
    ap.add_argument("--out-dir", default=None, help="where the FASTQ and BAM files go (default: <cache>/records_bench_<pid>; removed afterwards)")
    args = ap.parse_args()
    wl = bench.WORKLOADS[args.workload]
    lib = api.LIB_PATH = args.lib
    prefix = bench.prepare_index(args.cache, args.workload, wl["lens"], wl["seed"], wl["families"], 0, lambda: None, {}, alt_spec=wl.get("alt_spec"),
                                 decoy_spec=wl.get("decoy_spec"))
    rs = bench.workload_reads(wl, wl["seed"] + 1000, bench.load_genome(prefix), args.barcodes or wl["barcodes"], wl["ppb"])
    d = args.out_dir or os.path.join(args.cache, "records_bench_%d" % os.getpid())
    os.makedirs(d, exist_ok=True)
    plain = (os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq"))
    synth.write_fastq_fast(rs, *plain)
    for p in plain:                              # into the page cache
        with open(p, "rb") as f:
            while f.read(1 << 24):
                pass
    print(json.dumps(dict(what="input", workload=args.workload, pairs=rs.n_pairs)), flush=True)
    ref = api.Reference(prefix, lib_path=lib)
    rows = []
    try:
        # ---- kernels and traffic: the whole set as one batch
        fd = api.Feeder(*plain, lib_path=lib)
        sb, v = fd.next_raw(rs.n_pairs)
        P = int(v["n_pairs"])
        b = ref.batch(v["bases"], v["lens"]).run()
        n_cands = b.rfa(v["set_pair_off"], v["do_rfa"], fetch=False)
        b.post(fetch=False)
        n, nb = b.records(sb)                    # untimed: the phase's memory, the code objects
        ref.kernel_times_reset(True)
        for _ in range(args.repeats):
            b.records(sb)
        kt = ref.kernel_times()
        ref.kernel_times_reset(False)
        c = b.counts()
        n_bases = int(v["lens"].sum(dtype=np.int64))
        name_b, rg_b = int(np.frombuffer((api.C.c_int64 * (P + 1)).from_address(sb.name_off), dtype=np.int64)[-1]), int(np.frombuffer((api.C.c_int64 * (P + 1)).from_address(sb.rg_off), dtype=np.int64)[-1])
        per_call = {k: kt[k]["ms"] / kt[k]["calls"] for k in ("rec_size", "scan", "rec_tile", "rec_fill") if k in kt}
        # what the fill must move: every source byte once (names and read groups once per read of the pair), 96 bytes of RecMeta and an offset per record, the tile table; the stream out
        fill_read = 2 * n_bases + 2 * (name_b + rg_b) + 4 * c["n_cigar"] + (96 + 4) * n + 4 * ((nb + 255) // 256)
        fill_bw = (fill_read + nb) / (per_call["rec_fill"] * 1e-3) if per_call.get("rec_fill") else 0.0
        print(json.dumps(dict(what="kernels", pairs=P, records=n, stream_bytes=nb, ms_per_call={k: round(x, 4) for k, x in per_call.items()}, fill_bytes_read=fill_read,
                              fill_bytes_written=nb, fill_bytes_per_s=round(fill_bw), fill_fraction_of_peak=round(fill_bw / args.hbm_peak, 4), hbm_peak=args.hbm_peak)), flush=True)
        for k, x in per_call.items():
            rows.append((f"kernel {k}", f"{x:9.4f} ms per {P} pairs"))
        rows.append(("fill traffic", f"{(fill_read + nb) / 1e6:.1f} MB in {per_call.get('rec_fill', 0):.4f} ms = {fill_bw / 1e12:.3f} TB/s = {100 * fill_bw / args.hbm_peak:.1f} % of {args.hbm_peak / 1e12:.0f} TB/s"))
        # ---- PCIe bytes per 1 M pairs, from this batch's counts
        slabs = 4 * (2 * P + 1) + (api.REG_DTYPE.itemsize + api.ALN_DTYPE.itemsize) * c["n_regs"] + 4 * c["n_cigar"] + 4 * (2 * P + 1) + (api.CAND_DTYPE.itemsize + api.POST_DTYPE.itemsize) * n_cands
        up = n_bases + name_b + rg_b + 16 * (P + 1) + 17 * int(v["n_sets"]) + int(np.frombuffer((api.C.c_int64 * (int(v["n_sets"]) + 1)).from_address(sb.barcode_off), dtype=np.int64)[-1])
        scale = 1e6 / P
        pcie = {"records=host sink=host": dict(d2h=slabs, h2d=0), "records=host sink=device": dict(d2h=slabs, h2d=nb, note="plus the compressed blocks home"),
                "records=device sink=host": dict(d2h=nb, h2d=up), "records=device sink=device": dict(d2h=0, h2d=up, note="plus the compressed blocks home")}
        for k, x in pcie.items():
            x["d2h"], x["h2d"] = round(x["d2h"] * scale), round(x["h2d"] * scale)
            rows.append((f"PCIe per 1 M pairs, {k}", f"D2H {x['d2h'] / 1e6:8.1f} MB  H2D {x['h2d'] / 1e6:8.1f} MB  {x.get('note', '')}"))
        print(json.dumps(dict(what="pcie_per_1M_pairs", n_regs=c["n_regs"], n_cands=n_cands, arms=pcie)), flush=True)
        if args.layout == "reference":
            # ---- the full phase on the same batch: tags once, then arx_batch_records_full
            names, _, clens, _, _ = ref.contigs()
            table = api.bucket_table(names, clens, args.chunk, lib_path=lib)
            n_mm = b.post(fetch=False)               # (again, for the size of the mismatch lists; the tags go on top of it)
            b.tags(fetch=False)
            nf, nbf = b.records_full(sb, table)      # untimed
            ref.kernel_times_reset(True)
            for _ in range(args.repeats):
                b.records_full(sb, table)
            kt = ref.kernel_times()
            ref.kernel_times_reset(False)
            full_names = ("rec_mm_len", "rec_full_count", "rec_full_meta", "rec_tile", "rec_full_fill", "rec_group_count", "rec_group_rank", "rec_group_size", "rec_group_off", "scan")
            per_phase = {k: kt[k]["ms"] / args.repeats for k in full_names if k in kt}      # per records_full call (rec_tile / rec_full_fill run twice in it)
            print(json.dumps(dict(what="kernels_full", pairs=P, records=nf, stream_bytes=nbf, files=len(table.files), ms_per_phase={k: round(x, 4) for k, x in per_phase.items()},
                                  ms_total=round(sum(per_phase.values()), 4))), flush=True)
            for k, x in per_phase.items():
                rows.append((f"full phase {k}", f"{x:9.4f} ms per {P} pairs"))
            rows.append(("full phase stream", f"{nbf * scale / 1e6:.1f} MB per 1 M pairs, {nf} records, each written twice"))
            home = slabs + api.SPLIT_DTYPE.itemsize * 2 * P + 8 * n_mm + api.TAGS_DTYPE.itemsize * 2 * P
            upf = up + 4 * len(names)
            pcie = {"records=host sink=host": dict(d2h=home, h2d=0), "records=host sink=device": dict(d2h=home, h2d=2 * nbf, note="plus the compressed blocks home"),
                    "records=device_full sink=host": dict(d2h=2 * nbf + 16 * (len(table.files) + 1), h2d=upf),
                    "records=device_full sink=device": dict(d2h=16 * (len(table.files) + 1), h2d=upf, note="plus the compressed blocks home")}
            for k, x in pcie.items():
                x["d2h"], x["h2d"] = round(x["d2h"] * scale), round(x["h2d"] * scale)
                rows.append((f"PCIe per 1 M pairs (reference), {k}", f"D2H {x['d2h'] / 1e6:8.1f} MB  H2D {x['h2d'] / 1e6:8.1f} MB  {x.get('note', '')}"))
            print(json.dumps(dict(what="pcie_per_1M_pairs_reference", n_mm=n_mm, arms=pcie)), flush=True)
        b.free()
        fd.close()
        # ---- end to end, four arms
        if not args.no_e2e:
            kw = dict(pairs_per_batch=args.pairs_per_batch, bam_threads=8, rec_threads=8, lib_path=lib)
            if args.feeder == "device":
                kw.update(feeder="device", workers=args.workers)
            arms = [("host", "host"), ("device", "host"), ("host", "device"), ("device", "device")]
            if args.layout == "reference":
                arms = [("host", "host"), ("device_full", "host"), ("host", "device"), ("device_full", "device")]
                kw.update(layout="reference", chunk=args.chunk)
            res = {a: [] for a in arms}
            for rep in range(args.repeats + 1):          # pass 0 of every arm is not counted: it pays for the handles' work memory and the sink's buffers
                for records, sink in arms:
                    st = e2e.run(ref, [plain], os.path.join(d, f"out_{records}_{sink}"), records=records, sink=sink, **kw)
                    assert st["pairs"] == rs.n_pairs
                    print(json.dumps(dict(what="e2e", layout=args.layout, counted=rep > 0, records=records, sink=sink, feeder=args.feeder, workers=st["workers"], pairs=st["pairs"], seconds=round(st["seconds"], 4),
                                          pairs_per_s=round(st["pairs_per_s"]), worker_seconds={k: round(st[k], 3) for k in ("feeder_s", "device_s", "fetch_s", "records_s", "bam_s")})), flush=True)
                    if rep > 0:
                        res[records, sink].append(st["pairs_per_s"])
            for a in arms:
                x = sorted(res[a])
                rows.append((f"e2e records={a[0]} sink={a[1]}", f"{x[len(x) // 2] / 1e6:6.3f} M pairs/s  (min {x[0] / 1e6:.3f}, max {x[-1] / 1e6:.3f}, {len(x)} passes)"))
    finally:
        ref.close()
        if not args.out_dir:
            shutil.rmtree(d, ignore_errors=True)
    for what, val in rows:
        print(f"{what:44s} {val}", file=sys.stderr)


if __name__ == "__main__":
    main()

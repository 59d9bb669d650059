#!/usr/bin/env python3
"""Throughput of the BAM sink (arx_bam_*) on this host: typical 2x150 bp records (name, one CIGAR op, 150 bases + qualities, ~45 bytes
of aux), one batch of n records written `reps` times, for several thread counts.  Usage: bam_sink_bench.py [n_records] [threads ...]

--device [--level L] [--passes P] [--binned]: the same records through both sinks, alternating -- per pass the host sink (zlib level L, default 1)
at every thread count, then the device sink (arx_bam_open_device on device 0, a tiny index built on the spot; records encoded on the largest
thread count).  One JSON line per run: sink, threads, records/s, bytes per record in and out.  --binned: qualities binned to four levels
(.02/.05/.13/.8, with --device) instead of uniform 2..40."""
import json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C
import numpy as np
from arachne_amd import api

args = sys.argv[1:]
device = "--device" in args
binned = "--binned" in args
level, passes = 1, 5
for flag in ("--level", "--passes"):
    if flag in args:
        v = int(args[args.index(flag) + 1])
        del args[args.index(flag):args.index(flag) + 2]
        level, passes = (v, passes) if flag == "--level" else (level, v)
args = [a for a in args if not a.startswith("--")]
n = int(args[0]) if args else 400_000
threads = [int(x) for x in args[1:]] or ([1, 8, 16] if device else [1, 8, 32])
rng = np.random.default_rng(1)
names = [b"r%09d" % i for i in range(n)]
if device:   # byte-wide draws: the int64 index arrays of rng.choice would be 2.4 GB each at 2 M records
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, 150), dtype=np.uint8)]
    lut = np.full(256, 37 + 33, np.uint8); lut[:5] = 2 + 33; lut[5:18] = 12 + 33; lut[18:51] = 23 + 33      # .02 / .05 / .13 / .8
    qual = lut[rng.integers(0, 256, size=(n, 150), dtype=np.uint8)] if binned else (rng.integers(2, 41, size=(n, 150), dtype=np.uint8) + 33).astype(np.uint8)
else:
    seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(n, 150))
    qual = (rng.integers(2, 41, size=(n, 150)) + 33).astype(np.uint8)
aux1 = b"RGZlib1\0ASC\x96XMZ0\0AMZ1\0XTC\0BXZA01C02B03D04-1\0VXC\x01"
lib = api._load(api.LIB_PATH)
name_off = np.arange(n + 1, dtype=np.int64) * 10
name_b = np.frombuffer(b"".join(names), dtype=np.uint8)
flag = np.full(n, 99, np.int32); rid = np.zeros(n, np.int32); pos = rng.integers(0, 200_000_000, size=n).astype(np.int32); mapq = np.full(n, 60, np.uint8)
mrid = np.zeros(n, np.int32); mpos = pos + 200; tlen = np.full(n, 350, np.int32)
cig_off = np.arange(n + 1, dtype=np.int64); cig = np.full(n, 150 << 4, np.uint32)
seq_off = np.arange(n + 1, dtype=np.int64) * 150
aux_off = np.arange(n + 1, dtype=np.int64) * len(aux1); aux_b = np.frombuffer(aux1 * n, dtype=np.uint8)
b = api._BamBatch(n, name_off.ctypes.data, name_b.ctypes.data, flag.ctypes.data, rid.ctypes.data, pos.ctypes.data, mapq.ctypes.data, mrid.ctypes.data, mpos.ctypes.data,
                  tlen.ctypes.data, cig_off.ctypes.data, cig.ctypes.data, seq_off.ctypes.data, seq.ctypes.data, qual.ctypes.data, 33, aux_off.ctypes.data, aux_b.ctypes.data)
out = "/dev/shm/arx_bam_bench.bam" if os.path.isdir("/dev/shm") else "/tmp/arx_bam_bench.bam"
names_c = (C.c_char_p * 1)(b"chr1"); lens = np.array([248956422], np.int32)


def one(open_fn, reps):
    h = C.c_void_p(); msg = C.create_string_buffer(256)
    assert open_fn(h, msg) == 0, msg.value
    t0 = time.time()
    for _ in range(reps):
        assert lib.arx_bam_write(h, C.byref(b)) == 0
    st = np.zeros(4, np.int64)
    assert lib.arx_bam_close(h, st.ctypes.data) == 0
    return time.time() - t0, st


if not device:
    for t in threads:
        reps = 3
        dt, st = one(lambda h, msg: lib.arx_bam_open(out.encode(), 1, names_c, lens.ctypes.data, None, t, -1, C.byref(h), msg, 256), reps)
        print(f"{t:3d} threads: {reps * n / dt / 1e6:.2f} M records/s, {st[2] / dt / 1e6:.0f} MB/s in, {st[3] / dt / 1e6:.0f} MB/s out, ratio {st[2] / st[3]:.2f}")
    os.remove(out)
    sys.exit(0)

from arachne_amd import synth
d = tempfile.mkdtemp(prefix="arx_sink_bench_")
fa = os.path.join(d, "g.fa")
synth.make_genome(15, [200000]).write_fasta(fa)
api.index_build(fa, fa)
ref = api.Reference(fa)
open_dev = api._selftest_fn(ref.lib, "arx_bam_open_device")
enc = max(threads)
one(lambda h, msg: open_dev(ref.h, out.encode(), 1, names_c, lens.ctypes.data, None, enc, C.byref(h), msg, 256), 1)     # untimed: the first launch loads the code object
for p in range(passes):
    for t in threads:
        dt, st = one(lambda h, msg: lib.arx_bam_open(out.encode(), 1, names_c, lens.ctypes.data, None, t, level, C.byref(h), msg, 256), 1)
        print(json.dumps(dict(sink="host", threads=t, level=level, pass_=p, records=n, seconds=round(dt, 4), records_per_s=round(n / dt), bytes_in_per_record=round(st[2] / n, 2),
                              bytes_out_per_record=round(st[3] / n, 2))), flush=True)
    dt, st = one(lambda h, msg: open_dev(ref.h, out.encode(), 1, names_c, lens.ctypes.data, None, enc, C.byref(h), msg, 256), 1)
    print(json.dumps(dict(sink="device", threads=enc, pass_=p, records=n, seconds=round(dt, 4), records_per_s=round(n / dt), bytes_in_per_record=round(st[2] / n, 2),
                          bytes_out_per_record=round(st[3] / n, 2))), flush=True)
ref.close()
os.remove(out)

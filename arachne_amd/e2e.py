"""End to end: FASTQ pairs in, BAM files out -- the loop of the reference's Arachne() (src/aligner/aligner.go:335-371: a producer reading
barcode sets, `-t` workers calling DoRFAForOneBarcode, one BamThread writing, bamwriter.go:615-658) re-shaped around the device path.
Everything between the file reads and the file writes goes through the C ABI of include/arachne_amd.h; this module is the host-side
mirror of the Go driver (Python here because the image has no Go toolchain; INTEGRATION.md has the Go form).

ONE worker loop (run's `work`) serves every arm, on worker threads that live as long as the run.  Per super-batch (whole barcode sets, ~pairs_per_batch pairs) a worker takes it from its
source, loads it into its own batch handle, runs arx_batch_run / arx_batch_rfa on the handle's stream, hands it to the record mode, tells
the source that the feeder's arrays of it are free, and counts.  Four axes, each stated once:

  feeder   where super-batches come from.  "host" (_host_source): k file pairs, each with a worker and an arx_feeder of its own; loaded by
           arx_batch_reset.  "device" (_device_source): ONE file pair, the reference's own shape -- one producer thread with the device feeder
           (arx_feeder_open_device: two reader threads, the parse in HIP kernels) and `workers` workers that take its super-batches from a
           queue, the reads already in HBM (arx_feeder_device_reads -> arx_batch_reset_device).
  layout   where records go (_Sink).  "workers": one `<out_prefix>.k.bam` per worker with the primary record of every read.  "reference": the
           reference's output directory (CreateBAMs, bamwriter.go:127-190) -- bc_sorted_bam.bam, the position buckets of `chunk` bases and
           ZZZ_unmapped_pos_bucketed.bam -- with the reference's record set (split records, full tags), every record written twice, to
           bc_sorted_bam.bam and to its bucket (AppendBams, :279-281).  All workers append to shared writers, one lock per writer: a
           super-batch's records are contiguous and in order inside every file, the order of super-batches across workers is as arbitrary as
           the reference's goroutines make it.
  records  how records are made (_MODES, chosen from layout and records).  "host": arx_batch_fetch + arx_batch_rfa_fetch + arx_batch_post_fetch
           into reused host arrays, arx_recbuf_build / arx_recbuf_build_full on host threads, arx_bam_write on the worker's writer thread
           (_Writer).  "device" / "device_full": arx_batch_records / arx_batch_records_full encode them on the GPU.
  sink     how BGZF blocks are made: on the writers' host threads, or by HIP kernels (arx_bam_open_device)."""
from __future__ import annotations

import functools
import os
import queue
import threading
import time
import types

import numpy as np

from . import api

_TRACE = bool(os.environ.get("ARX_E2E_TRACE"))
_COUNTERS = dict(pairs=0, records=0, batches=0, feeder_s=0.0, device_s=0.0, fetch_s=0.0, records_s=0.0, bam_s=0.0)


def run(ref: api.Reference, fastq_pairs, out_prefix: str, pairs_per_batch: int = 250_000, bam_threads: int = 8, rec_threads: int = 8, level: int = 1,
        penalty: float = -4, lib_path: str = api.LIB_PATH, warm_passes: int = 0, layout: str = "workers", chunk: int = 40_000_000,
        read_groups: str = "", sample_id: str = "", feeder: str = "host", workers: int = 3, chunk_bytes: int = 0,
        sink: str = "host", records: str = "host", inflate: str = "host", final_bam: str | None = None, gunzip: str = "host"):
    """fastq_pairs: [(r1, r2), ...] barcode-sorted files (plain or gzip).  -> stats dict (pairs, records, batches, seconds, pairs/s, bam_bytes,
    workers, files, per-stage seconds summed over workers; bam_s: the writes and the closing of the writers).  One loop with four axes (the module docstring has them):
    feeder="host" (default): one host feeder and one worker per file pair.  feeder="device": ONE file pair, parsed on the GPU by one feeder
    thread (arx_feeder_open_device) that hands super-batches to `workers` worker threads; stats["feeder"] are the feeder's own counts.
    inflate="device" (feeder="device" only): BGZF files are inflated by a HIP kernel instead of zlib on the reader threads (api.Feeder).
    gunzip="device" (feeder="device" only): ordinary gzip files are inflated on the GPU in chunks, both files at once (api.Feeder); stats["gunzip"]
    are the two files' counts then.
    layout="workers" (default): out_prefix.k.bam per worker.  layout="reference": out_prefix is the output directory of the reference's layout
    (chunk = -p/--partitions, read_groups / sample_id as the reference's flags).
    records="host" (default): the records are built on host threads from the fetched result slabs.  records="device" (layout="workers" only):
    the primary records are encoded on the GPU (arx_batch_records); a worker fetches ONE block, the record stream, and queues it for its
    writer thread (arx_bam_write_encoded), or with sink="device" hands it to the device sink where it lies (arx_bam_write_encoded_device) -- the
    records never visit the host uncompressed.  arx_batch_post still runs, for the duplicate marks.  records="device_full" (layout="reference"
    only): the reference's record set and its buckets from the GPU (arx_batch_post, arx_batch_tags, arx_batch_records_full): the record stream
    goes to bc_sorted_bam.bam, every non-empty bucket's slice of the grouped stream to its writer -- fetched as two blocks, or with
    sink="device" handed over where they lie; no result slab comes home and nothing is built or encoded on host threads.  The files inflate to
    the same bytes in every mode; fetch_s / records_s are the stream fetch and post (+ tags) + the records call in the device modes.
    sink="device": every BAM writer compresses its BGZF blocks on ref's GPU (arx_bam_open_device; `level` does not apply); the files inflate
    to the same bytes as with the default, sink="host".
    warm_passes (host feeder, layout="workers" only): untimed passes over the same files first, through the same batch handles -- a handle's
    first batch pays for its work memory (hipMalloc of several GiB: seconds once a 69 GB k-mer table sits beside it), which a run over a
    whole read set pays once; the stats are those of the last pass.
    final_bam (layout="reference" only; default: off): after the pass, finalize() sorts the position buckets on ref's GPU into that one
    coordinate-sorted BAM, through a writer of the same `sink`; stats["final"] are its stats."""
    if final_bam is not None and layout != "reference":
        raise ValueError("final_bam is made from the position buckets: it needs layout='reference'")
    if sink not in ("host", "device"):
        raise ValueError(f"unknown sink {sink!r}")
    if records not in ("host", "device", "device_full"):
        raise ValueError(f"unknown records {records!r}")
    if records == "device" and layout == "reference":
        raise ValueError("records='device' writes the primary records only: layout='reference' needs records='host'")
    if records == "device_full" and layout != "reference":
        raise ValueError("records='device_full' builds the reference's record set and its buckets: it needs layout='reference'")
    if feeder not in ("host", "device"):
        raise ValueError(f"unknown feeder {feeder!r}")
    if inflate not in ("host", "device"):
        raise ValueError(f"unknown inflate {inflate!r}")
    if inflate == "device" and feeder != "device":
        raise ValueError("inflate='device' is the device feeder's: it needs feeder='device' (the host feeder inflates with zlib)")
    if gunzip not in ("host", "device"):
        raise ValueError(f"unknown gunzip {gunzip!r}")
    if gunzip == "device" and feeder != "device":
        raise ValueError("gunzip='device' is the device feeder's: it needs feeder='device' (the host feeder inflates with zlib)")
    if layout not in ("workers", "reference"):
        raise ValueError(f"unknown layout {layout!r}")
    if warm_passes and feeder == "device":
        raise ValueError("feeder='device' reads its file pair once: warm_passes must be 0")
    if warm_passes and layout == "reference":
        raise ValueError("layout='reference' writes its files once: warm_passes must be 0")
    if feeder == "device" and len(fastq_pairs) != 1:
        raise ValueError("feeder='device' takes exactly one file pair")
    if feeder == "device" and workers < 1:
        raise ValueError("workers must be at least 1")
    n_workers = workers if feeder == "device" else len(fastq_pairs)
    mode = _MODES[layout, records]
    sink_dev = ref if sink == "device" else None
    # what a worker keeps from pass to pass: its batch handle (the point of a warm pass), the arrays the slabs are fetched into, and two record
    # buffers -- one is written out while the next is built
    kept = []
    queued = records == "host" or (records, sink) == ("device", "host")         # the modes that write on a writer thread
    # the worker threads live as long as the handles: a warm pass leaves them where the timed pass finds them
    go, current = threading.Barrier(n_workers + 1), {}

    def body(k):
        try:
            for _ in range(warm_passes + 1):
                go.wait()
                current["work"](k)      # (catches what it raises)
                go.wait()
        except threading.BrokenBarrierError:
            pass
    pool = [threading.Thread(target=body, args=(k,)) for k in range(n_workers)]

    def one_pass():
        stats, lock, errors = dict(_COUNTERS), threading.Lock(), []
        out = _Sink(ref, layout, out_prefix, n_workers, chunk, read_groups, bam_threads, level, lib_path, sink_dev, own=(feeder, layout) == ("host", "workers"))
        take = producer = fd = None
        try:
            if feeder == "device":
                fd = api.Feeder(*fastq_pairs[0], device=ref, chunk_bytes=chunk_bytes, depth=n_workers + 2, inflate=inflate, gunzip=gunzip)
                take, producer = _device_source(ref, fd, pairs_per_batch, n_workers, errors, stats, lock)

            def work(k):
                w, close = kept[k], _nothing
                w.out, w.loc, w.streams = out, dict(_COUNTERS), [None, None]
                loc = w.loc
                try:
                    wr = w.wr = _Writer(loc) if queued else None
                    try:
                        nxt = take
                        if nxt is None:
                            nxt, close = _host_source(ref, *fastq_pairs[k], pairs_per_batch, lib_path)
                        out.open_own(k)
                        while not errors:
                            t0 = time.time()
                            item = nxt()
                            t1 = time.time()
                            if item is None:
                                break
                            sb, v, load, release = item
                            n_pairs = int(v["n_pairs"])
                            w.batch = load(w.batch)
                            w.batch.run(api.STAGE_ALN)
                            w.batch.rfa(v["set_pair_off"], v["do_rfa"], penalty=penalty, fetch=False)
                            t2 = time.time()
                            if _TRACE:
                                print(f"[e2e] worker {k} batch {loc['batches']}: {n_pairs} pairs, feeder {t1 - t0:.3f}s device {t2 - t1:.3f}s", flush=True)
                            n_rec = mode(w, w.batch, sb, loc["batches"] & 1)
                            # the records are built (and fetched or written): the feeder's arrays of this super-batch are free.  A mode that queues its
                            # write has done so: that put() never waits for a write (two slots, and the slot's last write was waited for before the
                            # build), so the producer is released when the records are built, as its gating rule has it
                            release()
                            loc["pairs"] += n_pairs; loc["records"] += n_rec; loc["batches"] += 1
                            loc["device_s"] += t2 - t1
                            if producer is None:            # (the device feeder's seconds are its producer's)
                                loc["feeder_s"] += t1 - t0
                    finally:
                        if wr is not None:
                            wr.end()
                        t5 = time.time()
                        out.close_own(k)
                        loc["bam_s"] += time.time() - t5
                        close()
                    if wr is not None:
                        wr.check()
                except BaseException as e:  # noqa: BLE001 -- reported by the caller's thread
                    errors.append(e)
                with lock:
                    for key, val in loc.items():
                        stats[key] += val

            th = [threading.Thread(target=producer)] if producer else []
            current["work"] = work
            t = time.time()
            for x in th:
                x.start()
            go.wait()                   # the pass starts
            go.wait()                   # ... and is over when every worker is through (and has closed its own BAM)
            for x in th:
                x.join()
        finally:
            t5 = time.time()
            stats["bam_bytes"] = out.close()
            stats["bam_s"] += time.time() - t5
            if fd is not None:
                fd.close()
        if errors:
            raise errors[0]
        # the span of a pass: a worker's own files (host feeder, layout="workers") are opened and closed inside it, the shared ones are opened
        # in front of it and closed inside it
        stats["seconds"] = time.time() - t
        stats["pairs_per_s"] = stats["pairs"] / stats["seconds"] if stats["seconds"] > 0 else 0.0
        stats.update(warm_passes=warm_passes, workers=n_workers, files=out.files)
        return stats

    try:
        for x in pool:
            x.start()
        for k in range(n_workers):
            kept.append(types.SimpleNamespace(k=k, batch=None, buf={}, rb=[api.RecBuf(lib_path=lib_path), api.RecBuf(lib_path=lib_path)], rec_threads=rec_threads))
        for _ in range(warm_passes + 1):
            stats = one_pass()
    finally:
        go.abort()
        for x in pool:
            x.join()
        for w in kept:
            if w.batch is not None:
                w.batch.free()
            for x in w.rb:
                x.free()
    if final_bam is not None:
        stats["final"] = finalize(ref, out_prefix, final_bam, sink=sink, chunk=chunk, read_groups=read_groups, bam_threads=bam_threads, level=level, lib_path=lib_path)
    return stats


def finalize(ref: api.Reference, out_dir: str, final_path: str, sink: str = "host", chunk: int = 40_000_000, read_groups: str = "", bam_threads: int = 8,
             level: int = 1, max_bytes: int = 0, lib_path: str = api.LIB_PATH, index: "bool | str" = False, index_pass: str = "separate"):
    """The step the position buckets exist for: out_dir is a reference-layout directory (run(layout="reference") with the same chunk); every
    bucket of api.bucket_table that was written is sorted by coordinate on ref's GPU (BamWriter.sort_append) and appended, in table order, to ONE
    writer with reference_header(read_groups) and SO:coordinate; the unmapped file, which is its own sorted form (refID = pos = -1 throughout),
    is appended in copy mode.  Buckets hold disjoint, ascending ranges of (contig, position), so the concatenation is sorted.  sink as in run.
    -> dict(records, buckets, bytes, seconds, sort: the per-file stats).  index=True: the closed file's .bai is written beside it
    (final_path + ".bai", api.bam_index on ref's device -- one more read of the file); the dict gains index (its stats) and index_seconds.
    index="bai" is the same, and like the other names adds index_format ("bai" or "csi": what was written); "csi" writes final_path + ".csi" (api.bam_index_csi), the index that holds contigs above 2^29
    bases, which api.bam_index refuses; "auto" writes the .csi where a contig exceeds 2^29 and the .bai otherwise.
    index_pass="writer" (with an index): the writer itself indexes what it appends, on ref's GPU, and writes the index when it is closed
    (api.BamWriter(index=...)) -- the same BAM and the same index bytes without the second read of the file; index, index_format and
    index_seconds (the time the writer spent indexing) come from the close.  "separate", the default, is the pass described above."""
    if sink not in ("host", "device"):
        raise ValueError(f"unknown sink {sink!r}")
    if not (index is False or index is True or index in ("bai", "csi", "auto")):
        raise ValueError(f"unknown index {index!r}")
    if index_pass not in ("separate", "writer"):
        raise ValueError(f"unknown index_pass {index_pass!r}")
    in_writer = bool(index) and index_pass == "writer"
    names, offs, clens, alt, l_pac = ref.contigs()
    table = api.bucket_table(names, clens, chunk, lib_path=lib_path)
    t = time.time()
    w = api.BamWriter(final_path, names, clens, extra_header=reference_header(read_groups), threads=bam_threads, level=level, lib_path=lib_path,
                      device=ref if sink == "device" else None, coordinate=True, **(dict(index="bai" if index is True else index, index_device=ref) if in_writer else {}))
    per = []
    try:
        for k, f in enumerate(table.files):
            p = os.path.join(out_dir, f)
            if not os.path.exists(p):       # a bucket that was never written
                continue
            unmapped = k == len(table.files) - 1
            per.append(dict(file=f, **w.sort_append(ref, p, mode="copy" if unmapped else "coordinate", max_bytes=max_bytes)))
    finally:
        st = w.close()
    out = dict(records=st["records"], buckets=len(per), bytes=st["bytes_out"], seconds=time.time() - t, sort=per)
    if in_writer:
        out["index"], out["index_seconds"] = st["index"], st["index"]["total_us"] / 1e6
        if index is not True:
            out["index_format"] = st["index_format"]
    elif index:
        fmt = "bai" if index is True else index
        if fmt == "auto":
            fmt = "csi" if any(int(l) > api.BAI_MAX_CONTIG for l in clens) else "bai"
        t = time.time()
        out["index"] = (api.bam_index_csi if fmt == "csi" else api.bam_index)(final_path, device=ref.device, lib_path=lib_path)
        out["index_seconds"] = time.time() - t
        if index is not True:               # a format that was asked for by name is named in the answer; True answers as it always has
            out["index_format"] = fmt
    return out


def standardize(r1: str, r2: str, out_dir: str, format="auto", bgzf: bool = False, device: int = 0, lib_path: str = api.LIB_PATH, gunzip: str = "host"):
    """The step in front of presort(): a haplotagging, stLFR or TELLseq pair with its headers rewritten on the GPU to the BX:Z: / VX:i: form the
    feeder and the sort read (api.fastq_standardize; the reference's half-written standardize.go).  format "auto" detects from the first 200
    records; a pair that is standard already is returned as it is.  The rewritten files go to out_dir under the inputs' base names
    (+ ".std.fastq", ".gz" with bgzf).  gunzip="device": ordinary gzip inputs are inflated on the GPU (api.fastq_standardize).
    -> (r1_std, r2_std, stats); stats["standardized"] says whether files were written."""
    def name(p):
        b = os.path.basename(p)
        for ext in (".gz", ".bgz", ".fastq", ".fq"):
            if b.endswith(ext):
                b = b[:-len(ext)]
        return os.path.join(out_dir, b + ".std.fastq" + (".gz" if bgzf else ""))
    if api._fqstd_format(format) == 0:
        st = api.fastq_standardize(r1, r2, detect=True, device=device, lib_path=lib_path, gunzip=gunzip)
        if st["format"] == "standard":
            return r1, r2, dict(st, standardized=False)
        if st["format"] != "unknown":
            format = st["format"]       # detected once; "unknown" goes on to the call, whose error says what to do
    os.makedirs(out_dir, exist_ok=True)
    o1, o2 = name(r1), name(r2)
    if o1 == o2:
        o2 = o2.replace(".std.", ".std.2.")
    st = api.fastq_standardize(r1, r2, o1, o2, format=format, bgzf=bgzf, device=device, lib_path=lib_path, gunzip=gunzip)
    return o1, o2, dict(st, standardized=True)


def presort(r1: str, r2: str, out_dir: str, device: int = 0, bgzf: bool = False, if_needed: bool = True, lib_path: str = api.LIB_PATH, run_bytes: int = 0,
            tmp_dir: "str | None" = None, gunzip: str = "host"):
    """The step in front of run(): the file pair sorted by barcode on the GPU (api.fastq_sort; the reference's `arachne preprocess`), which
    the feeder's barcode sets rely on.  With if_needed the input is counted first (check=True) and returned as it is when every barcode
    is one run already.  The sorted files go to out_dir under the inputs' base names (+ ".sorted.fastq", ".gz" with bgzf: a BGZF file is a
    gzip file).  run_bytes != 0 sorts in runs of that many bytes per file through temporary files under tmp_dir (api.fastq_sort_ex: a pair that
    device memory does not hold; -1: the library chooses), the count before it included.  gunzip="device": ordinary gzip inputs are inflated on
    the GPU (api.fastq_sort).
    -> (r1_sorted, r2_sorted, stats); stats["sorted"] says whether files were written."""
    sort = api.fastq_sort if run_bytes == 0 else functools.partial(api.fastq_sort_ex, run_bytes=run_bytes, tmp_dir=tmp_dir)
    if if_needed:
        st = sort(r1, r2, check=True, device=device, lib_path=lib_path, gunzip=gunzip)
        if st["runs"] == st["distinct"]:
            return r1, r2, dict(st, sorted=False)
    os.makedirs(out_dir, exist_ok=True)

    def name(p):
        b = os.path.basename(p)
        for ext in (".gz", ".bgz", ".fastq", ".fq"):
            if b.endswith(ext):
                b = b[:-len(ext)]
        return os.path.join(out_dir, b + ".sorted.fastq" + (".gz" if bgzf else ""))
    o1, o2 = name(r1), name(r2)
    if o1 == o2:
        o2 = o2.replace(".sorted.", ".sorted.2.")
    st = sort(r1, r2, o1, o2, bgzf=bgzf, device=device, lib_path=lib_path, gunzip=gunzip)
    return o1, o2, dict(st, sorted=True)


def prepare(r1: str, r2: str, out_dir: str, format="auto", bgzf: bool = False, device: int = 0, run_bytes: int = 0, tmp_dir: "str | None" = None, if_needed: bool = True,
            lib_path: str = api.LIB_PATH, gunzip: str = "host"):
    """standardize() and presort() as one GPU call (api.fastq_prepare), without the files between them: the pair comes out with the headers the
    feeder reads, ordered by barcode.  With if_needed the input is counted first (check=True) and returned as it is when its format is the
    standard one and every key is one run already; a pair in another format is always written, its headers have to change.  The files go to
    out_dir under the inputs' base names (+ ".prepared.fastq", ".gz" with bgzf).  run_bytes, tmp_dir and gunzip as in presort().
    -> (r1_out, r2_out, stats); stats["prepared"] says whether files were written."""
    if if_needed:
        st = api.fastq_prepare(r1, r2, format=format, check=True, run_bytes=run_bytes, device=device, lib_path=lib_path, gunzip=gunzip)
        if st["format"] == "standard" and st["runs"] == st["distinct"]:
            return r1, r2, dict(st, prepared=False)
        format = st["format"]               # detected once
    os.makedirs(out_dir, exist_ok=True)

    def name(p):
        b = os.path.basename(p)
        for ext in (".gz", ".bgz", ".fastq", ".fq"):
            if b.endswith(ext):
                b = b[:-len(ext)]
        return os.path.join(out_dir, b + ".prepared.fastq" + (".gz" if bgzf else ""))
    o1, o2 = name(r1), name(r2)
    if o1 == o2:
        o2 = o2.replace(".prepared.", ".prepared.2.")
    st = api.fastq_prepare(r1, r2, o1, o2, format="auto" if format == "standard" else format, bgzf=bgzf, run_bytes=run_bytes, tmp_dir=tmp_dir, device=device, lib_path=lib_path,
                           gunzip=gunzip)
    return o1, o2, dict(st, prepared=True)


def _nothing():
    pass


# ---- feeder: where super-batches come from.  A source is a call -> None at the end, or (sb, v, load, release): the super-batch and its views,
# load(batch or None) -> the batch handle with these reads in it, release() once the feeder's arrays of this super-batch are no longer needed
def _host_source(ref, r1, r2, pairs_per_batch, lib_path):
    """-> (source, close): a worker's own host feeder; its arrays hold until the worker's next call, so there is nothing to release"""
    fd = api.Feeder(r1, r2, lib_path=lib_path)

    def take():
        nx = fd.next_raw(pairs_per_batch)
        if nx is None:
            return None
        sb, v = nx

        def load(batch):
            return batch.reset(v["bases"], v["lens"]) if batch is not None else ref.batch(v["bases"], v["lens"])
        return sb, v, load, _nothing
    return take, fd.close


def _device_source(ref, fd, pairs_per_batch, workers, errors, stats, lock):
    """-> (source, producer): the reference's shape (aligner.go:335-358) -- ONE producer thread with the device feeder fd, whose parse runs on
    the GPU, puts super-batches into a queue, every worker takes them from it (arx_batch_reset_device from the feeder's device arrays: the
    bases never come back to the host for the path's sake).  Which worker takes which super-batch is as free as it is across the reference's
    goroutines.  The producer's seconds in the feeder go to stats["feeder_s"], the feeder's counts to stats["feeder"]."""
    # The feeder recycles its arrays by AGE: those of its call k hold until its call k + depth returns, however many newer super-batches are
    # done with.  So the producer makes call m only when every super-batch up to m - depth has been released by its worker (done[j], set
    # once the records are built): it runs at most depth - 1 calls ahead of the oldest one in use, and a worker that is held up in one
    # super-batch stops the producer, not the feeder's arrays under it.  depth = workers + 2: one per worker, one in the queue, one in the making.
    depth = workers + 2
    done = []                           # done[j]: the worker that took super-batch j no longer needs the feeder's arrays of it
    q = queue.Queue(maxsize=1)
    stats["feeder"] = {}

    def producer():
        try:
            while not errors:
                m = len(done)
                while m >= depth and not done[m - depth].wait(0.2):
                    if errors:
                        return
                t0 = time.time()
                nx = fd.next_raw(pairs_per_batch)
                if nx is None:
                    break
                done.append(threading.Event())
                item = nx + (fd.device_reads(), done[m])
                with lock:
                    stats["feeder_s"] += time.time() - t0
                while not errors:
                    try:
                        q.put(item, timeout=0.2)
                        break
                    except queue.Full:
                        pass
            stats["feeder"].update(fd.stats())
            if fd.gunzip == "device":
                stats["gunzip"] = list(fd.gunzip_stats())
        except BaseException as e:  # noqa: BLE001 -- reported by the caller's thread
            errors.append(e)
        finally:
            for _ in range(workers):
                while True:
                    try:
                        q.put(None, timeout=0.2)
                        break
                    except queue.Full:
                        if errors:
                            try:
                                q.get_nowait()
                            except queue.Empty:
                                pass

    def take():
        item = q.get()
        if item is None:
            return None
        sb, v, (d_bases, d_lens, n_bases), released = item

        def load(batch):
            if batch is None:
                batch = ref.batch(np.zeros(2, np.uint8), np.ones(2, np.int32))          # a handle; its reads come from the device below
            return batch.reset_device(2 * int(v["n_pairs"]), n_bases, d_bases, d_lens)
        return sb, v, load, released.set
    return take, producer


# ---- layout: where records go
class _Sink:
    """The BAM writers of one pass, a lock for each and, for layout="reference", the bucket table.  A call writes one super-batch's records
    under the lock of every writer it appends to: they are contiguous and in order in every file.  own: writer k is worker k's alone (host
    feeder, layout="workers") -- that worker opens and closes it (open_own, close_own), side by side with the others; else all are opened here
    and closed by close()."""

    def __init__(self, ref, layout, out, n_workers, chunk, read_groups, bam_threads, level, lib_path, device, own):
        names, offs, clens, alt, l_pac = ref.contigs()
        self.device, self.table, self.own = device, None, own
        if layout == "reference":
            self.table = api.bucket_table(names, clens, chunk, lib_path=lib_path)
            os.makedirs(out, exist_ok=True)
            self.files = ["bc_sorted_bam.bam"] + self.table.files
            paths, hdr = [os.path.join(out, f) for f in self.files], reference_header(read_groups)
        else:
            self.files = paths = [f"{out}.{k}.bam" for k in range(n_workers)]
            hdr = "@PG\tID:arachne_amd\n"
        self.locks = [threading.Lock() for _ in paths]
        self.writers, self.bytes = [None] * len(paths), [0] * len(paths)
        self._open = lambda k: api.BamWriter(paths[k], names, clens, extra_header=hdr, threads=bam_threads, level=level, lib_path=lib_path, device=device)
        try:
            for k in range(0 if own else len(paths)):
                self.writers[k] = self._open(k)
        except BaseException:
            self.close()
            raise

    def open_own(self, k):
        if self.own:
            self.writers[k] = self._open(k)

    def close_own(self, k):
        if self.own and self.writers[k] is not None:
            w, self.writers[k] = self.writers[k], None
            self.bytes[k] = w.close()["bytes_out"]

    def view(self, k, view, bucket):
        """a host-built view from worker k: into its file, or (bucket: the bucket of every record) into bc_sorted_bam.bam and the buckets"""
        if self.table is None:
            with self.locks[k]:
                self.writers[k].write_view(view)
            return
        order = np.argsort(bucket, kind="stable")
        cuts = np.searchsorted(bucket[order], np.arange(len(self.table.files) + 1))
        with self.locks[0]:
            self.writers[0].write_view(view)
        self._buckets(cuts, lambda w, f: w.write_select(view, order[cuts[f]:cuts[f + 1]]))

    def stream(self, k, data, n_rec, n_bytes=None):
        """an encoded stream from worker k, into its file or bc_sorted_bam.bam: host bytes, or with n_bytes a device pointer (device sink only)"""
        i = k if self.table is None else 0
        with self.locks[i]:
            if n_bytes is None:
                self.writers[i].write_encoded(data, n_rec)
            else:
                self.writers[i].write_encoded_device(data, n_bytes, n_rec)

    def grouped(self, data, bo, ro, device=False):
        """the grouped stream, bucket f's records ro[f]:ro[f + 1] in bytes bo[f]:bo[f + 1]: host bytes, or a device pointer (device sink only)"""
        if device:
            self._buckets(ro, lambda w, f: w.write_encoded_device(data + int(bo[f]), int(bo[f + 1] - bo[f]), int(ro[f + 1] - ro[f])))
        else:
            self._buckets(ro, lambda w, f: w.write_encoded(data[bo[f]:bo[f + 1]], int(ro[f + 1] - ro[f])))

    def _buckets(self, off, write):
        """write(writer, f) for every non-empty bucket f (AppendBams, bamwriter.go:279-281)"""
        for f in range(len(self.table.files)):
            if off[f + 1] > off[f]:
                with self.locks[f + 1]:
                    write(self.writers[f + 1], f)

    def close(self):
        """closes every writer that is still open, whatever happens to one of them -> bytes written, by all of them"""
        err = None
        for k, w in enumerate(self.writers):
            try:
                if w is not None:
                    self.writers[k] = None
                    self.bytes[k] = w.close()["bytes_out"]
            except BaseException as e:  # noqa: BLE001
                err = err or e
        if err is not None:
            raise err
        return sum(self.bytes)


# ---- the writer thread
class _Writer:
    """A worker's BamThread (bamwriter.go:615-658): what is put() is compressed and written by a thread of its own while the worker goes on with
    the next barcode sets.  Two slots: the buffers behind slot s are reused two super-batches later, after wait(s) -- its write has returned.
    A failed write is raised by the worker's next wait() or by check(); end() always ends the thread."""

    def __init__(self, loc):
        self.loc, self.err, self.q = loc, [], queue.Queue(maxsize=1)
        self.written = [threading.Event(), threading.Event()]
        for e in self.written:
            e.set()
        self.thread = threading.Thread(target=self._run)
        self.thread.start()

    def _run(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            slot, write = item
            try:
                t = time.time()
                write()
                self.loc["bam_s"] += time.time() - t
            except BaseException as e:  # noqa: BLE001 -- raised in the worker
                self.err.append(e)
            finally:
                self.written[slot].set()

    def wait(self, slot):
        self.written[slot].wait()                       # the slot's last write is on disk
        self.check()

    def check(self):
        if self.err:
            raise self.err[0]

    def put(self, slot, write):
        self.written[slot].clear()
        self.q.put((slot, write))

    def end(self):
        self.q.put(None)
        self.thread.join()


# ---- records: how records are made.  mode(w, batch, sb, slot) -> records, for the super-batch sb that run and rfa are done with on worker w's
# batch; adds its seconds to w.loc and writes through w.out, on the writer thread w.wr or here
def _host_primary(w, batch, sb, slot):
    t2, b = time.time(), w.buf
    batch.fetch_into(b)
    post = batch.post_into(b)
    t3 = time.time()
    w.wr.wait(slot)
    view = w.rb[slot].build(sb, b["cand_off"], b["cands"], b["alns"], b["cigars"], post, threads=w.rec_threads)
    w.loc["fetch_s"] += t3 - t2; w.loc["records_s"] += time.time() - t3
    w.wr.put(slot, lambda: w.out.view(w.k, view, None))
    return int(view.n_records)


def _host_full(w, batch, sb, slot):
    t2, b = time.time(), w.buf
    batch.fetch_into(b)
    post = batch.post()                                 # arx_batch_post, then the tags on top of it (a later post would discard them)
    tags = batch.tags()
    t3 = time.time()
    w.wr.wait(slot)
    view, bucket = w.rb[slot].build_full(sb, b["cand_off"], b["cands"], b["alns"], b["cigars"], post["post"], post["split"], post["mm_ref"], post["mm_read"],
                                         tags, w.out.table, threads=w.rec_threads)
    bucket = bucket.copy()                              # the record buffer's own array: rebuilt before this write may have read it
    w.loc["fetch_s"] += t3 - t2; w.loc["records_s"] += time.time() - t3
    w.wr.put(slot, lambda: w.out.view(w.k, view, bucket))
    return int(view.n_records)


def _pinned(w, batch, slot, n_bytes):
    """w.streams[slot], a page-locked host buffer for an encoded stream, grown when needed (the old one is dropped before the new one is pinned)"""
    if w.streams[slot] is None or len(w.streams[slot]) < n_bytes:
        w.streams[slot] = None
        w.streams[slot] = batch.pin(np.zeros(int(n_bytes * 1.2) + 4096, dtype=np.uint8))
    return w.streams[slot]


def _device_primary(w, batch, sb, slot):
    """the stream into the device sink where it lies (the call returns when its blocks are written: the batch may be reset), or home as one
    block, one buffer written out while the next is fetched"""
    t2 = time.time()
    batch.post(fetch=False)                             # for the duplicate marks
    n_rec, n_bytes = batch.records(sb)
    t3 = time.time()
    w.loc["records_s"] += t3 - t2
    if w.out.device is not None:
        ptr, n_bytes, n_rec = batch.records_view()
        w.out.stream(w.k, ptr, n_rec, n_bytes)
        w.loc["bam_s"] += time.time() - t3
        return n_rec
    w.wr.wait(slot)
    stream, _ = batch.records_fetch(out=_pinned(w, batch, slot, n_bytes), offsets=False)
    w.loc["fetch_s"] += time.time() - t3
    w.wr.put(slot, lambda: w.out.stream(w.k, stream, n_rec))
    return n_rec


def _device_full(w, batch, sb, slot):
    """the record stream and the grouped stream from device memory with the device sink, else fetched as two blocks and written here: returns
    when the writers have taken the bytes"""
    t2 = time.time()
    batch.post(fetch=False)                             # arx_batch_post, then the tags on top of it (a later post would discard them)
    batch.tags(fetch=False)
    n_rec, n_bytes = batch.records_full(sb, w.out.table)
    t3 = time.time()
    w.loc["records_s"] += t3 - t2
    if w.out.device is not None:
        ptr, n_bytes, n_rec = batch.records_view()
        gptr, bo, ro = batch.records_buckets_view()
        w.out.stream(w.k, ptr, n_rec, n_bytes)
        w.out.grouped(gptr, bo, ro, device=True)
        w.loc["bam_s"] += time.time() - t3
        return n_rec
    bufs = [_pinned(w, batch, s, n_bytes) for s in (0, 1)]
    stream, _ = batch.records_fetch(out=bufs[0], offsets=False)
    g = batch.records_buckets_fetch(out=bufs[1], bucket=False)
    t4 = time.time()
    w.loc["fetch_s"] += t4 - t3
    w.out.stream(w.k, stream, n_rec)
    w.out.grouped(g["grouped"], g["byte_off"], g["rec_off"])
    w.loc["bam_s"] += time.time() - t4
    return n_rec


_MODES = {("workers", "host"): _host_primary, ("workers", "device"): _device_primary, ("reference", "host"): _host_full, ("reference", "device_full"): _device_full}


def reference_header(read_groups: str = "", date: str | None = None) -> str:
    """The header lines CreateBAM adds to every file (bamwriter.go:74-109): one @RG per comma-separated read group of at least five ':' fields
    (sample:library:gem_group:flowcell:lane -> ID, LB = library.gem_group, PL ILLUMINA, PU = ID, SM = sample, DT = the run time), then @PG."""
    if date is None:
        date = time.strftime("%Y-%m-%dT%H:%M:%S%z")
    out = ""
    for rg in read_groups.split(",") if read_groups else []:
        f = rg.split(":")
        if len(f) < 5:
            continue
        out += f"@RG\tID:{rg}\tPL:ILLUMINA\tPU:{rg}\tLB:{f[1]}.{f[2]}\tSM:{f[0]}\tDT:{date}\n"
    return out + "@PG\tID:arachne\tPN:arachne\tCL:arachne_amd\n"

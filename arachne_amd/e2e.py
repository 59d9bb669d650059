"""End to end: FASTQ pairs in, BAM files out -- the loop of the reference's Arachne() (src/aligner/aligner.go:335-371: a producer reading
barcode sets, `-t` workers calling DoRFAForOneBarcode, one BamThread writing, bamwriter.go:615-658) re-shaped around the device path:

    k file pairs, each with its own worker thread:
        arx_feeder_next (whole barcode sets, ~pairs_per_batch pairs)  ->  arx_batch_reset / run / rfa / post on the worker's own stream
        ->  arx_batch_fetch + arx_batch_rfa_fetch + arx_batch_post_fetch into reused host arrays  ->  arx_recbuf_build (AppendBam's record
        logic on host threads)  ->  arx_bam_write (BGZF on host threads) into the worker's own BAM

Everything between the file reads and the file writes goes through the C ABI of include/arachne_amd.h; this module is the host-side
mirror of the Go driver (Python here because the image has no Go toolchain; INTEGRATION.md has the Go form).

Two layouts.  layout="workers" (the default): one `<out_prefix>.k.bam` per worker with the primary record of every read (arx_recbuf_build).
layout="reference": the reference's output directory (CreateBAMs, bamwriter.go:127-190) -- bc_sorted_bam.bam, the position buckets of
`chunk` bases and ZZZ_unmapped_pos_bucketed.bam -- with the reference's record set (arx_batch_tags + arx_recbuf_build_full: split records,
full tags) and every record written twice, to bc_sorted_bam.bam and to its bucket (AppendBams, :279-281).  All workers append to shared
writers, one lock per writer: a batch's records are contiguous and in order inside every file, the order of batches across workers is
as arbitrary as the reference's goroutines make it.

feeder="device" (opt in): ONE file pair, the reference's own shape -- one producer thread with the device feeder (arx_feeder_open_device: two
reader threads, the parse in HIP kernels) and `workers` worker threads that take its super-batches from a queue, the reads already in HBM
(arx_feeder_device_reads -> arx_batch_reset_device); see _run_device.
"""
from __future__ import annotations

import threading
import time

import os

import numpy as np

from . import api

_TRACE = bool(os.environ.get("ARX_E2E_TRACE"))


def run(ref: api.Reference, fastq_pairs, out_prefix: str, pairs_per_batch: int = 250_000, bam_threads: int = 8, rec_threads: int = 8, level: int = 1,
        penalty: float = -4, lib_path: str = api.LIB_PATH, warm_passes: int = 0, layout: str = "workers", chunk: int = 40_000_000,
        read_groups: str = "", sample_id: str = "", feeder: str = "host", workers: int = 3, chunk_bytes: int = 0,
        sink: str = "host", records: str = "host"):
    """fastq_pairs: [(r1, r2), ...] barcode-sorted files (plain or gzip), one worker each.  -> stats dict (pairs, seconds, pairs/s, per-stage
    seconds summed over workers).  warm_passes: untimed passes over the same files first, through the same batch handles -- a handle's first
    batch pays for its work memory (hipMalloc of several GiB: seconds once a 69 GB k-mer table sits beside it), which a run over a whole
    read set pays once; the stats are those of the last pass.  layout="reference": out_prefix is the output directory of the reference's
    layout (see the module docstring; chunk = -p/--partitions, read_groups / sample_id as the reference's flags); warm_passes must be 0.
    feeder="device": ONE file pair, parsed on the GPU by one feeder thread (arx_feeder_open_device) that hands super-batches to `workers`
    worker threads (see _run_device); the default, feeder="host", is one host feeder and one worker per file pair.
    sink="device": every BAM writer, in both layouts, compresses its BGZF blocks on ref's GPU (arx_bam_open_device; `level` does not apply); the
    files inflate to the same bytes as with the default, sink="host".
    records="device" (layout="workers" only, both feeders): the BAM records are encoded on the GPU (arx_batch_records) instead of fetching the
    result slabs and building them on host threads (arx_recbuf_build + arx_bam_write's encoder): a worker fetches ONE block, the record
    stream, and queues it for its writer thread (arx_bam_write_encoded), or with sink="device" hands it to the device sink where it lies
    (arx_bam_write_encoded_device) -- the records never visit the host uncompressed.  arx_batch_post still runs, for the duplicate marks.  The
    files inflate to the same bytes; fetch_s / records_s then are the stream fetch and post + the records call.
    records="device_full" (layout="reference" only, both feeders): the reference's record set and its buckets from the GPU
    (arx_batch_post, arx_batch_tags, arx_batch_records_full): the record stream goes to bc_sorted_bam.bam, every non-empty bucket's slice of
    the grouped stream to its writer -- fetched as two blocks (arx_bam_write_encoded), or with sink="device" handed over where they lie
    (arx_bam_write_encoded_device); no result slab comes home and nothing is built or encoded on host threads."""
    if sink not in ("host", "device"):
        raise ValueError(f"unknown sink {sink!r}")
    if records not in ("host", "device", "device_full"):
        raise ValueError(f"unknown records {records!r}")
    if records == "device" and layout == "reference":
        raise ValueError("records='device' writes the primary records only: layout='reference' needs records='host'")
    if records == "device_full" and layout != "reference":
        raise ValueError("records='device_full' builds the reference's record set and its buckets: it needs layout='reference'")
    dev_rec = "full" if records == "device_full" else records == "device"
    sink_dev = ref if sink == "device" else None
    if feeder == "device":
        if warm_passes:
            raise ValueError("feeder='device' reads its file pair once: warm_passes must be 0")
        return _run_device(ref, fastq_pairs, out_prefix, pairs_per_batch, bam_threads, rec_threads, level, penalty, lib_path, layout, chunk, read_groups, workers, chunk_bytes, sink_dev, dev_rec)
    if feeder != "host":
        raise ValueError(f"unknown feeder {feeder!r}")
    if layout == "reference":
        if warm_passes:
            raise ValueError("layout='reference' writes its files once: warm_passes must be 0")
        return _run_reference(ref, fastq_pairs, out_prefix, pairs_per_batch, bam_threads, rec_threads, level, penalty, lib_path, chunk, read_groups, sample_id, sink_dev, dev_rec == "full")
    if layout != "workers":
        raise ValueError(f"unknown layout {layout!r}")
    names, offs, clens, alt, l_pac = ref.contigs()
    stats = dict(pairs=0, records=0, batches=0, feeder_s=0.0, device_s=0.0, fetch_s=0.0, records_s=0.0, bam_s=0.0)
    lock = threading.Lock()
    errors = []

    gate = threading.Barrier(len(fastq_pairs) + 1)
    t_pass = [0.0] * (warm_passes + 2)

    def worker(k, r1, r2):
        try:
            batch, buf = None, {}
            rb = [api.RecBuf(lib_path=lib_path), api.RecBuf(lib_path=lib_path)]   # two record buffers: one is written out while the next is built
            for ps in range(warm_passes + 1):
                gate.wait()
                batch, buf = one_pass(k, r1, r2, batch, buf, rb, ps == warm_passes)
                gate.wait()
            if batch is not None:
                batch.free()
            for x in rb:
                x.free()
        except BaseException as e:  # noqa: BLE001 -- reported by the caller's thread
            errors.append(e)
            gate.abort()

    def one_pass(k, r1, r2, batch, buf, rb, counted):
        if True:
            fd = api.Feeder(r1, r2, lib_path=lib_path)
            bam = api.BamWriter(f"{out_prefix}.{k}.bam", names, clens, extra_header="@PG\tID:arachne_amd\n", threads=bam_threads, level=level, lib_path=lib_path, device=sink_dev)
            loc = dict(pairs=0, records=0, batches=0, feeder_s=0.0, device_s=0.0, fetch_s=0.0, records_s=0.0, bam_s=0.0)
            # the worker's BamThread (bamwriter.go:615-658): record views are compressed and written by a thread of their own while the worker
            # goes on with the next barcode sets; a view's record buffer is reused two batches later, when its write has returned
            import queue
            wq = queue.Queue(maxsize=1)
            written = [threading.Event(), threading.Event()]
            for e_ in written:
                e_.set()
            werr = []
            streams = [None, None]                      # records="device": two host buffers for the record stream, one written out while the next is fetched

            def writer():
                while True:
                    item = wq.get()
                    if item is None:
                        return
                    slot, write = item
                    try:
                        t_ = time.time()
                        write()
                        loc["bam_s"] += time.time() - t_
                    except BaseException as e:  # noqa: BLE001
                        werr.append(e)
                    finally:
                        written[slot].set()
            wt = threading.Thread(target=writer)
            wt.start()
            while True:
                t0 = time.time()
                nx = fd.next_raw(pairs_per_batch)
                t1 = time.time()
                if nx is None:
                    break
                sb, v = nx
                batch = batch.reset(v["bases"], v["lens"]) if batch is not None else ref.batch(v["bases"], v["lens"])
                batch.run(api.STAGE_ALN)
                batch.rfa(v["set_pair_off"], v["do_rfa"], penalty=penalty, fetch=False)
                t2 = time.time()
                if _TRACE:
                    print(f"[e2e] worker {k} batch {loc['batches']}: {int(v['n_pairs'])} pairs, feeder {t1 - t0:.3f}s device {t2 - t1:.3f}s", flush=True)
                slot = loc["batches"] & 1
                if dev_rec:
                    n_rec = _device_records(batch, sb, bam, sink_dev, slot, written, werr, wq, streams, loc)
                    loc["pairs"] += int(v["n_pairs"]); loc["records"] += n_rec; loc["batches"] += 1
                    loc["feeder_s"] += t1 - t0; loc["device_s"] += t2 - t1
                    continue
                batch.fetch_into(buf)
                post = batch.post_into(buf)
                t3 = time.time()
                written[slot].wait()                    # the buffer's last view is on disk
                if werr:
                    raise werr[0]
                view = rb[slot].build(sb, buf["cand_off"], buf["cands"], buf["alns"], buf["cigars"], post, threads=rec_threads)
                t4 = time.time()
                written[slot].clear()
                wq.put((slot, lambda view=view: bam.write_view(view)))
                loc["pairs"] += int(v["n_pairs"]); loc["records"] += int(view.n_records); loc["batches"] += 1
                loc["feeder_s"] += t1 - t0; loc["device_s"] += t2 - t1; loc["fetch_s"] += t3 - t2; loc["records_s"] += t4 - t3
            wq.put(None)
            wt.join()
            if werr:
                raise werr[0]
            t5 = time.time()
            st = bam.close()
            loc["bam_s"] += time.time() - t5
            fd.close()
            if counted:
                with lock:
                    for key, val in loc.items():
                        stats[key] += val
                    stats.setdefault("bam_bytes", 0)
                    stats["bam_bytes"] += st["bytes_out"]
            return batch, buf

    th = [threading.Thread(target=worker, args=(k, r1, r2)) for k, (r1, r2) in enumerate(fastq_pairs)]
    for x in th:
        x.start()
    t = time.time()
    try:
        for ps in range(warm_passes + 1):
            gate.wait()                 # the pass starts
            t = time.time()
            gate.wait()                 # ... and is over when every worker has closed its BAM
            t_pass[ps] = time.time() - t
    except threading.BrokenBarrierError:
        pass
    for x in th:
        x.join()
    if errors:
        raise errors[0]
    stats["seconds"] = t_pass[warm_passes]
    stats["warm_passes"] = warm_passes
    stats["pairs_per_s"] = stats["pairs"] / stats["seconds"] if stats["seconds"] > 0 else 0.0
    stats["workers"] = len(fastq_pairs)
    return stats


def _device_records(batch, sb, bam, sink_dev, slot, written, werr, wq, streams, loc, lock=None):
    """records="device" for one super-batch of a worker: arx_batch_post (duplicate marks), arx_batch_records, then the stream either into the
    device sink where it lies (the call returns when its blocks are written: the batch may be reset) or home as one block into streams[slot]
    and onto the worker's writer thread.  -> records written"""
    import contextlib
    t2 = time.time()
    batch.post(fetch=False)
    n_rec, n_bytes = batch.records(sb)
    t3 = time.time()
    loc["records_s"] += t3 - t2
    guard = lock if lock is not None else contextlib.nullcontext()
    if sink_dev is not None:
        ptr, n_bytes, n_rec = batch.records_view()
        with guard:
            bam.write_encoded_device(ptr, n_bytes, n_rec)
        loc["bam_s"] += time.time() - t3
        return n_rec
    written[slot].wait()                                # the buffer's last stream is on disk
    if werr:
        raise werr[0]
    if streams[slot] is None or len(streams[slot]) < n_bytes:
        streams[slot] = None
        streams[slot] = batch.pin(np.zeros(int(n_bytes * 1.2) + 4096, dtype=np.uint8))
    stream, _ = batch.records_fetch(out=streams[slot], offsets=False)
    loc["fetch_s"] += time.time() - t3
    written[slot].clear()

    def write():
        with guard:
            bam.write_encoded(stream, n_rec)
    wq.put((slot, write))
    return n_rec


def _device_records_full(batch, sb, table, writers, locks, sink_dev, streams, loc):
    """records="device_full" for one super-batch: arx_batch_post, arx_batch_tags, arx_batch_records_full, then the record stream into writers[0]
    (bc_sorted_bam.bam) and bucket f's slice of the grouped stream into writers[f + 1] (AppendBams, bamwriter.go:279-281) -- from device memory
    with the device sink, else fetched as two blocks into streams[0] / streams[1] (page-locked, grown when needed).  Returns when the
    writers have taken the bytes: the batch may be reset.  -> records"""
    t2 = time.time()
    batch.post(fetch=False)                             # arx_batch_post, then the tags on top of it (a later post would discard them)
    batch.tags(fetch=False)
    n_rec, n_bytes = batch.records_full(sb, table)
    t3 = time.time()
    loc["records_s"] += t3 - t2
    if sink_dev is not None:
        ptr, n_bytes, n_rec = batch.records_view()
        gptr, bo, ro = batch.records_buckets_view()
        with locks[0]:
            writers[0].write_encoded_device(ptr, n_bytes, n_rec)
        for f in range(len(table.files)):
            if ro[f + 1] > ro[f]:
                with locks[f + 1]:
                    writers[f + 1].write_encoded_device(gptr + int(bo[f]), int(bo[f + 1] - bo[f]), int(ro[f + 1] - ro[f]))
        loc["bam_s"] += time.time() - t3
        return n_rec
    for k in (0, 1):
        if streams[k] is None or len(streams[k]) < n_bytes:
            streams[k] = None
            streams[k] = batch.pin(np.zeros(int(n_bytes * 1.2) + 4096, dtype=np.uint8))
    stream, _ = batch.records_fetch(out=streams[0], offsets=False)
    g = batch.records_buckets_fetch(out=streams[1], bucket=False)
    t4 = time.time()
    loc["fetch_s"] += t4 - t3
    bo, ro = g["byte_off"], g["rec_off"]
    with locks[0]:
        writers[0].write_encoded(stream, n_rec)
    for f in range(len(table.files)):
        if ro[f + 1] > ro[f]:
            with locks[f + 1]:
                writers[f + 1].write_encoded(g["grouped"][bo[f]:bo[f + 1]], int(ro[f + 1] - ro[f]))
    loc["bam_s"] += time.time() - t4
    return n_rec


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


def _run_reference(ref, fastq_pairs, out_dir, pairs_per_batch, bam_threads, rec_threads, level, penalty, lib_path, chunk, read_groups, sample_id, sink_dev=None, full_dev=False):
    names, offs, clens, alt, l_pac = ref.contigs()
    table = api.bucket_table(names, clens, chunk, lib_path=lib_path)
    os.makedirs(out_dir, exist_ok=True)
    hdr = reference_header(read_groups)
    files = ["bc_sorted_bam.bam"] + table.files
    writers = [api.BamWriter(os.path.join(out_dir, f), names, clens, extra_header=hdr, threads=bam_threads, level=level, lib_path=lib_path, device=sink_dev) for f in files]
    locks = [threading.Lock() for _ in writers]
    stats = dict(pairs=0, records=0, batches=0, feeder_s=0.0, device_s=0.0, fetch_s=0.0, records_s=0.0, bam_s=0.0)
    slock = threading.Lock()
    errors = []

    def worker(k, r1, r2):
        batch = None
        fd = api.Feeder(r1, r2, lib_path=lib_path)
        rb = api.RecBuf(lib_path=lib_path)
        loc = dict(pairs=0, records=0, batches=0, feeder_s=0.0, device_s=0.0, fetch_s=0.0, records_s=0.0, bam_s=0.0)
        buf = {}
        streams = [None, None]
        try:
            while True:
                t0 = time.time()
                nx = fd.next_raw(pairs_per_batch)
                t1 = time.time()
                if nx is None:
                    break
                sb, v = nx
                batch = batch.reset(v["bases"], v["lens"]) if batch is not None else ref.batch(v["bases"], v["lens"])
                batch.run(api.STAGE_ALN)
                batch.rfa(v["set_pair_off"], v["do_rfa"], penalty=penalty, fetch=False)
                t2 = time.time()
                if full_dev:
                    n_rec = _device_records_full(batch, sb, table, writers, locks, sink_dev, streams, loc)
                    loc["pairs"] += int(v["n_pairs"]); loc["records"] += n_rec; loc["batches"] += 1
                    loc["feeder_s"] += t1 - t0; loc["device_s"] += t2 - t1
                    continue
                batch.fetch_into(buf)
                post = batch.post()                      # arx_batch_post, then the tags on top of it (a later post would discard them)
                tags = batch.tags()
                t3 = time.time()
                view, bucket = rb.build_full(sb, buf["cand_off"], buf["cands"], buf["alns"], buf["cigars"], post["post"], post["split"], post["mm_ref"],
                                             post["mm_read"], tags, table, threads=rec_threads)
                order = np.argsort(bucket, kind="stable")
                cuts = np.searchsorted(bucket[order], np.arange(len(table.files) + 1))
                t4 = time.time()
                with locks[0]:
                    writers[0].write_view(view)
                for f in range(len(table.files)):
                    if cuts[f + 1] > cuts[f]:
                        with locks[f + 1]:
                            writers[f + 1].write_select(view, order[cuts[f]:cuts[f + 1]])
                t5 = time.time()
                loc["pairs"] += int(v["n_pairs"]); loc["records"] += int(view.n_records); loc["batches"] += 1
                loc["feeder_s"] += t1 - t0; loc["device_s"] += t2 - t1; loc["fetch_s"] += t3 - t2; loc["records_s"] += t4 - t3; loc["bam_s"] += t5 - t4
        except BaseException as e:  # noqa: BLE001 -- reported by the caller's thread
            errors.append(e)
        finally:
            if batch is not None:
                batch.free()
            rb.free()
            fd.close()
        with slock:
            for key, val in loc.items():
                stats[key] += val

    t = time.time()
    th = [threading.Thread(target=worker, args=(k, r1, r2)) for k, (r1, r2) in enumerate(fastq_pairs)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    t5 = time.time()
    stats["bam_bytes"] = 0
    for w in writers:
        stats["bam_bytes"] += w.close()["bytes_out"]
    stats["bam_s"] += time.time() - t5
    if errors:
        raise errors[0]
    stats["seconds"] = time.time() - t
    stats["warm_passes"] = 0
    stats["pairs_per_s"] = stats["pairs"] / stats["seconds"] if stats["seconds"] > 0 else 0.0
    stats["workers"] = len(fastq_pairs)
    stats["files"] = files
    return stats


def _run_device(ref, fastq_pairs, out, pairs_per_batch, bam_threads, rec_threads, level, penalty, lib_path, layout, chunk, read_groups, workers, chunk_bytes, sink_dev=None, dev_rec=False):
    """One file pair, the reference's shape (aligner.go:335-358): ONE producer -- the device feeder, whose parse runs on the GPU -- puts
    super-batches into a queue, `workers` threads take them, each with its own batch handle (arx_batch_reset_device from the feeder's device
    arrays: the bases never come back to the host for the path's sake) and everything after that as in the host-feeder loops above.
    layout="workers": worker k writes `<out>.k.bam`; layout="reference": all workers append to the reference's files.  A super-batch's
    records stay contiguous and in order; which worker takes which super-batch is as free as it is across the reference's goroutines."""
    import queue
    if len(fastq_pairs) != 1:
        raise ValueError("feeder='device' takes exactly one file pair")
    if layout not in ("workers", "reference"):
        raise ValueError(f"unknown layout {layout!r}")
    if workers < 1:
        raise ValueError("workers must be at least 1")
    r1, r2 = fastq_pairs[0]
    names, offs, clens, alt, l_pac = ref.contigs()
    full = layout == "reference"
    if full:
        table = api.bucket_table(names, clens, chunk, lib_path=lib_path)
        os.makedirs(out, exist_ok=True)
        files = ["bc_sorted_bam.bam"] + table.files
        hdr = reference_header(read_groups)
        writers = [api.BamWriter(os.path.join(out, f), names, clens, extra_header=hdr, threads=bam_threads, level=level, lib_path=lib_path, device=sink_dev) for f in files]
    else:
        files = [f"{out}.{k}.bam" for k in range(workers)]
        writers = [api.BamWriter(f, names, clens, extra_header="@PG\tID:arachne_amd\n", threads=bam_threads, level=level, lib_path=lib_path, device=sink_dev) for f in files]
    locks = [threading.Lock() for _ in writers]
    stats = dict(pairs=0, records=0, batches=0, feeder_s=0.0, device_s=0.0, fetch_s=0.0, records_s=0.0, bam_s=0.0)
    slock = threading.Lock()
    errors = []
    # The feeder recycles its arrays by AGE: those of its call k hold until its call k + depth returns, however many newer super-batches are
    # done with.  So the producer makes call m only when every super-batch up to m - depth has been released by its worker (done[j], set
    # once the records are built): it runs at most depth - 1 calls ahead of the oldest one in use, and a worker that is held up in one
    # super-batch stops the producer, not the feeder's arrays under it.  depth = workers + 2: one per worker, one in the queue, one in the making.
    depth = workers + 2
    done = []                           # done[j]: the worker that took super-batch j no longer needs the feeder's arrays of it
    q = queue.Queue(maxsize=1)
    fd = api.Feeder(r1, r2, device=ref, chunk_bytes=chunk_bytes, depth=depth)
    feeder_stats = {}

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
                with slock:
                    stats["feeder_s"] += time.time() - t0
                while not errors:
                    try:
                        q.put(item, timeout=0.2)
                        break
                    except queue.Full:
                        pass
            feeder_stats.update(fd.stats())
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

    def worker(k):
        batch = None
        rb = [api.RecBuf(lib_path=lib_path), api.RecBuf(lib_path=lib_path)]     # one is written out while the next is built
        loc = dict(pairs=0, records=0, batches=0, device_s=0.0, fetch_s=0.0, records_s=0.0, bam_s=0.0)
        buf = {}
        wq = queue.Queue(maxsize=1)
        written = [threading.Event(), threading.Event()]
        for e_ in written:
            e_.set()
        werr = []
        streams = [None, None]

        def write(view, bucket):
            if not full:
                with locks[k]:
                    writers[k].write_view(view)
                return
            order = np.argsort(bucket, kind="stable")
            cuts = np.searchsorted(bucket[order], np.arange(len(table.files) + 1))
            with locks[0]:
                writers[0].write_view(view)
            for f in range(len(table.files)):
                if cuts[f + 1] > cuts[f]:
                    with locks[f + 1]:
                        writers[f + 1].write_select(view, order[cuts[f]:cuts[f + 1]])

        def writer():
            while True:
                item = wq.get()
                if item is None:
                    return
                slot, wr = item
                try:
                    t_ = time.time()
                    wr()
                    loc["bam_s"] += time.time() - t_
                except BaseException as e:  # noqa: BLE001
                    werr.append(e)
                finally:
                    written[slot].set()
        wt = threading.Thread(target=writer)
        wt.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                if errors:
                    continue
                sb, v, (d_bases, d_lens, n_bases), released = item
                t1 = time.time()
                if batch is None:
                    batch = ref.batch(np.zeros(2, np.uint8), np.ones(2, np.int32))      # a handle; its reads come from the device below
                batch.reset_device(2 * int(v["n_pairs"]), n_bases, d_bases, d_lens)
                batch.run(api.STAGE_ALN)
                batch.rfa(v["set_pair_off"], v["do_rfa"], penalty=penalty, fetch=False)
                t2 = time.time()
                if dev_rec == "full":
                    n_pairs = int(v["n_pairs"])
                    n_rec = _device_records_full(batch, sb, table, writers, locks, sink_dev, streams, loc)
                    released.set()                      # both streams are with their writers: the feeder's arrays are free
                    loc["pairs"] += n_pairs; loc["records"] += n_rec; loc["batches"] += 1
                    loc["device_s"] += t2 - t1
                    continue
                if dev_rec:
                    n_pairs = int(v["n_pairs"])
                    n_rec = _device_records(batch, sb, writers[k], sink_dev, loc["batches"] & 1, written, werr, wq, streams, loc, lock=locks[k])
                    released.set()                      # the stream is built (and fetched or compressed): the feeder's arrays are free
                    loc["pairs"] += n_pairs; loc["records"] += n_rec; loc["batches"] += 1
                    loc["device_s"] += t2 - t1
                    continue
                batch.fetch_into(buf)
                if full:
                    post = batch.post()
                    tags = batch.tags()
                else:
                    post = batch.post_into(buf)
                t3 = time.time()
                slot = loc["batches"] & 1
                written[slot].wait()                    # the buffer's last view is on disk
                if werr:
                    raise werr[0]
                if full:
                    view, bucket = rb[slot].build_full(sb, buf["cand_off"], buf["cands"], buf["alns"], buf["cigars"], post["post"], post["split"], post["mm_ref"],
                                                       post["mm_read"], tags, table, threads=rec_threads)
                    bucket = bucket.copy()
                else:
                    view, bucket = rb[slot].build(sb, buf["cand_off"], buf["cands"], buf["alns"], buf["cigars"], post, threads=rec_threads), None
                n_pairs = int(v["n_pairs"])
                released.set()                          # the feeder's arrays of this super-batch are no longer needed
                t4 = time.time()
                written[slot].clear()
                wq.put((slot, lambda view=view, bucket=bucket: write(view, bucket)))
                loc["pairs"] += n_pairs; loc["records"] += int(view.n_records); loc["batches"] += 1
                loc["device_s"] += t2 - t1; loc["fetch_s"] += t3 - t2; loc["records_s"] += t4 - t3
        except BaseException as e:  # noqa: BLE001 -- reported by the caller's thread
            errors.append(e)
        finally:
            wq.put(None)
            wt.join()
            if werr and not errors:
                errors.append(werr[0])
            if batch is not None:
                batch.free()
            for x in rb:
                x.free()
        with slock:
            for key, val in loc.items():
                stats[key] += val

    t = time.time()
    th = [threading.Thread(target=producer)] + [threading.Thread(target=worker, args=(k,)) for k in range(workers)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    t5 = time.time()
    stats["bam_bytes"] = 0
    for w in writers:
        stats["bam_bytes"] += w.close()["bytes_out"]
    stats["bam_s"] += time.time() - t5
    fd.close()
    if errors:
        raise errors[0]
    stats["seconds"] = time.time() - t
    stats["warm_passes"] = 0
    stats["pairs_per_s"] = stats["pairs"] / stats["seconds"] if stats["seconds"] > 0 else 0.0
    stats["workers"] = workers
    stats["files"] = files
    stats["feeder"] = feeder_stats
    return stats

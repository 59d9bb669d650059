"""Every arm of e2e.run on the host test double -- feeder x layout x records, the host sink -- against pinned digests of the files it writes
(tests/golden/e2e_arms_v1.json), and the way a run ends when a worker fails.

Ordered: one worker, so every file's bytes behind the BAM header are fixed (the header carries the run's time); sha256 of them, 16 hex digits.
Unordered: several workers, so only each file's multiset of records is fixed; sha256 over the records sorted as byte strings, each preceded by
its length as 4 little-endian bytes.  With the device feeder and layout="workers" which worker takes which super-batch is free: the records
of all files are pooled.  GPU variant, with the device sink: tests/test_e2e_arms_gpu.py."""
import hashlib
import json
import os
import struct
import subprocess
import tempfile
import threading
import time

import pytest

from arachne_amd import api, e2e, synth
import reccases as rc
import recfullcases as fc
import test_bam_reference_layout as trl

HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "hostsim", "libarx_hostsim.so")
GOLDEN = os.path.join(HERE, "golden", "e2e_arms_v1.json")
ARMS = [(feeder, layout, records) for feeder in ("host", "device") for layout, full in (("workers", "device"), ("reference", "device_full")) for records in ("host", full)]
BATCH_SIZES = (70, 45)                                                  # 300 pairs in barcode sets of 60: 4 and 6 super-batches


def body_digest(path):
    data = rc.inflate(path)
    return hashlib.sha256(data[rc.header_len(data):]).hexdigest()[:16]


def records_digest(recs):
    h = hashlib.sha256()
    for r in sorted(recs):
        h.update(struct.pack("<I", len(r)) + r)
    return h.hexdigest()[:16]


def split_files(rs, d, parts, tag):
    """the read set as `parts` FASTQ file pairs cut at barcode boundaries"""
    po = rs.pair_offsets()
    cuts = [int(po[len(po) * k // parts]) for k in range(parts)] + [rs.n_pairs]
    files = []
    for k in range(parts):
        f1, f2 = os.path.join(d, f"{tag}1_{k}.fq"), os.path.join(d, f"{tag}2_{k}.fq")
        synth.write_fastq_fast(rs, f1, f2, cuts[k], cuts[k + 1])
        files.append((f1, f2))
    return files


def run_arm(w, feeder, layout, records, order, ppb, tag=""):
    """-> (stats, paths).  ordered: the whole set as one pair, one worker.  unordered: two pairs with the host feeder, one pair and two workers with the
    device feeder"""
    out = os.path.join(w["d"], f"{tag}{order}_{feeder}_{layout}_{records}_{ppb}")
    files, extra = w["one"], {}
    if feeder == "device":
        extra = dict(feeder="device", workers=1 if order == "ordered" else 2)
    elif order == "unordered":
        files = w["two"]
    st = e2e.run(w["ref"], files, out, pairs_per_batch=ppb, bam_threads=2, rec_threads=3, lib_path=SIM, layout=layout, chunk=fc.CHUNK, records=records, **extra)
    return st, fc.e2e_paths(st, layout, out)


def unordered_digests(layout, paths):
    """-> {name: [digest, records]}; layout="workers": one entry, "records", over all files"""
    recs = {f: fc.records_of(p) for f, p in paths.items()}
    if layout == "workers":
        recs = {"records": [r for f in sorted(recs) for r in recs[f]]}
    return {f: [records_digest(r), len(r)] for f, r in recs.items()}


def make_world(d):
    g, rs = trl._reads(5, 60)                                           # 300 pairs; 615 records in the full set: split records are present
    fa = rc.make_index(d, g, SIM)
    return dict(d=d, rs=rs, one=split_files(rs, d, 1, "a"), two=split_files(rs, d, 2, "b"), ref=api.Reference(fa, lib_path=SIM))


@pytest.fixture(scope="module")
def world(built):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    w = make_world(tempfile.mkdtemp(prefix="arx_arms_"))
    w["golden"] = json.load(open(GOLDEN))
    yield w
    w["ref"].close()


def _check_stats(w, st, feeder, layout):
    n_pairs = w["rs"].n_pairs
    assert st["pairs"] == n_pairs and st["batches"] >= 4
    assert st["records"] == (w["golden"]["full_records"] if layout == "reference" else 2 * n_pairs)
    assert set(st) >= set(w["golden"]["keys"][f"{feeder}_{layout}"]), sorted(st)


@pytest.mark.parametrize("feeder,layout,records", ARMS)
def test_ordered_arm_writes_the_pinned_bytes(world, feeder, layout, records):
    want = world["golden"]["ordered"][layout]
    for ppb in BATCH_SIZES:
        st, paths = run_arm(world, feeder, layout, records, "ordered", ppb)
        _check_stats(world, st, feeder, layout)
        assert {f: body_digest(p) for f, p in paths.items()} == want, ppb


@pytest.mark.parametrize("feeder,layout,records", ARMS)
def test_unordered_arm_writes_the_pinned_records(world, feeder, layout, records):
    want = world["golden"]["unordered"][layout]
    for ppb in BATCH_SIZES:
        st, paths = run_arm(world, feeder, layout, records, "unordered", ppb)
        _check_stats(world, st, feeder, layout)
        assert st["workers"] == 2
        assert unordered_digests(layout, paths) == want, ppb


@pytest.mark.parametrize("layout,records,cls,method", [("workers", "host", "RecBuf", "build"), ("workers", "device", "Batch", "records"),
                                                       ("reference", "host", "RecBuf", "build_full")])
def test_an_error_ends_the_run_cleanly(world, monkeypatch, layout, records, cls, method):
    """the named call raises the second time it is made, in whichever worker makes it: e2e.run raises that exception, leaves no thread behind and
    every file closed.  The run has a thread of its own and every wait here a deadline: a loop that hangs fails this test, it does not hold it."""
    real = getattr(getattr(api, cls), method)
    calls, lock = [0], threading.Lock()

    def planted(self, *a, **kw):
        with lock:
            calls[0] += 1
            n = calls[0]
        if n == 2:
            raise RuntimeError("planted failure")
        return real(self, *a, **kw)
    monkeypatch.setattr(getattr(api, cls), method, planted)
    out = os.path.join(world["d"], f"err_{layout}_{records}")
    before = threading.active_count()
    caught = []

    def call():
        try:
            e2e.run(world["ref"], world["two"], out, pairs_per_batch=45, bam_threads=2, rec_threads=3, lib_path=SIM, layout=layout, chunk=fc.CHUNK, records=records)
        except BaseException as e:  # noqa: BLE001 -- looked at below
            caught.append(e)
    t = threading.Thread(target=call, daemon=True)
    t.start()
    t.join(60)
    assert not t.is_alive(), "e2e.run did not return"
    assert len(caught) == 1 and isinstance(caught[0], RuntimeError) and "planted failure" in str(caught[0]), caught
    deadline = time.time() + 5
    while threading.active_count() > before and time.time() < deadline:
        time.sleep(0.02)
    assert threading.active_count() == before, [x.name for x in threading.enumerate()]
    paths = [os.path.join(out, f) for f in os.listdir(out)] if layout == "reference" else [f"{out}.0.bam", f"{out}.1.bam"]
    assert len(paths) >= 2
    for p in paths:
        with open(p, "rb") as f:
            f.read()
        os.remove(p)

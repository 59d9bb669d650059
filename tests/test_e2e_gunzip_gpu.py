"""e2e.run with the device feeder's gzip input inflated on the GPU (gunzip="device": ARX_FEEDER_GUNZIP_DEVICE) against the same run with zlib on
the reader threads (gunzip="host"), on the small genome and 2,000 pairs of tests/test_e2e_arms_gpu.py's kind as one gzip pair: the same BAM,
record for record (two workers: which worker's file a super-batch goes to is free, so the records of all files together are compared)."""
import gzip
import os
import tempfile

import pytest

import reccases as rc
import recfullcases as fc
import test_bam_reference_layout as trl
from arachne_amd import api, e2e, synth

pytestmark = pytest.mark.gpu


def test_gunzip_on_the_device_writes_the_same_records():
    g, rs = trl._reads(10, 200)                                     # 2000 pairs, chimeras among them
    d = tempfile.mkdtemp(prefix="arx_e2e_gunzip_")
    fa = rc.make_index(d, g, api.LIB_PATH)
    f1, f2 = os.path.join(d, "b1.fq"), os.path.join(d, "b2.fq")
    synth.write_fastq_fast(rs, f1, f2)
    pair = []
    for f in (f1, f2):
        with open(f, "rb") as src, open(f + ".gz", "wb") as dst:
            dst.write(gzip.compress(src.read(), 6))
        pair.append(f + ".gz")
    ref = api.Reference(fa)
    try:
        got = {}
        for gunzip in ("host", "device"):
            o = os.path.join(d, gunzip)
            st = e2e.run(ref, [tuple(pair)], o, pairs_per_batch=600, bam_threads=2, rec_threads=3, feeder="device", workers=2, gunzip=gunzip)
            assert st["pairs"] == rs.n_pairs and st["records"] == 2 * rs.n_pairs and st["batches"] >= 3
            if gunzip == "device":
                for gs in st["gunzip"]:
                    assert gs["launches"] >= 1 and gs["accepted"] >= gs["launches"] and gs["host_bytes"] == 0 and gs["fallback"] == 0 and gs["members"] == 1, gs
            else:
                assert "gunzip" not in st
            got[gunzip] = sorted(r for p in fc.e2e_paths(st, "workers", o).values() for r in fc.records_of(p))
        assert len(got["host"]) == 2 * rs.n_pairs and got["device"] == got["host"]
        with pytest.raises(ValueError):
            e2e.run(ref, [tuple(pair)], os.path.join(d, "refused"), gunzip="device")          # the host feeder inflates with zlib
    finally:
        ref.close()

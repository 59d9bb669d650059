"""Every arm of e2e.run on the GPU: per (layout, feeder) the four arms records x sink, each held file by file to the records="host",
sink="host" arm of the same run.  4000 pairs with chimeras in super-batches of about 600: at least six of them, so both buffer slots of
every worker are reused -- where a lifetime mistake in the hand-off to the writer thread would show.  One pair and one worker with the host
feeder: the bytes behind the BAM header are identical.  Two workers with the device feeder: the same multiset of records (over all files
with layout="workers", where a super-batch goes to whichever worker is free).  Host-double variant, against pinned digests:
tests/test_e2e_arms.py."""
import os
import tempfile

import pytest

import reccases as rc
import recfullcases as fc
import test_bam_reference_layout as trl
from arachne_amd import api, e2e, synth

pytestmark = pytest.mark.gpu
LIB = api.LIB_PATH


@pytest.fixture(scope="module")
def big():
    g, rs = trl._reads(20, 200)                                     # 4000 pairs, chimeras among them, on a 550 kb genome
    d = tempfile.mkdtemp(prefix="arx_arms_gpu_")
    fa = rc.make_index(d, g, LIB)
    f1, f2 = os.path.join(d, "b1.fq"), os.path.join(d, "b2.fq")
    synth.write_fastq_fast(rs, f1, f2)
    ref = api.Reference(fa)
    yield dict(rs=rs, d=d, files=(f1, f2), ref=ref)
    ref.close()


@pytest.mark.parametrize("layout", ["workers", "reference"])
@pytest.mark.parametrize("feeder", ["host", "device"])
def test_every_arm_writes_what_the_host_arm_writes(big, feeder, layout):
    ref, d, rs = big["ref"], big["d"], big["rs"]
    extra = dict(feeder="device", workers=2) if feeder == "device" else {}
    got = {}
    for records in ("host", "device_full" if layout == "reference" else "device"):
        for sink in ("host", "device"):
            o = os.path.join(d, f"{feeder}_{layout}_{records}_{sink}")
            st = e2e.run(ref, [big["files"]], o, pairs_per_batch=600, bam_threads=2, rec_threads=3, layout=layout, chunk=fc.CHUNK, records=records, sink=sink, **extra)
            assert st["pairs"] == rs.n_pairs and st["batches"] >= 6
            assert st["records"] > 2 * rs.n_pairs if layout == "reference" else st["records"] == 2 * rs.n_pairs
            paths = fc.e2e_paths(st, layout, o)
            main = [paths["bc_sorted_bam.bam"]] if layout == "reference" else list(paths.values())
            assert max(len(rc.inflate(p)) for p in main) > 65280    # whole BGZF blocks went through the sink
            if feeder == "host":
                files = {f: rc.inflate(p) for f, p in paths.items()}
                got[records, sink] = {f: data[rc.header_len(data):] for f, data in files.items()}      # (the header carries the run's time)
            elif layout == "reference":
                got[records, sink] = {f: sorted(fc.records_of(p)) for f, p in paths.items()}
            else:
                got[records, sink] = {"records": sorted(r for p in paths.values() for r in fc.records_of(p))}
    want = got.pop(("host", "host"))
    assert len(got) == 3 and sum(len(x) for x in want.values()) > 0
    for arm, files in got.items():
        assert sorted(files) == sorted(want), arm
        for f in want:
            assert files[f] == want[f], (arm, f)

"""End to end from BGZF input with the inflate on the GPU (e2e.run(feeder="device", inflate="device")): one small pair; the BAM files
inflate to the same bytes as those of the run on the plain files."""
import os
import tempfile

import pytest

import bgzfio
import devfeed
from arachne_amd import api, e2e, synth

pytestmark = pytest.mark.gpu


def test_bgzf_input_inflated_on_the_device_gives_the_plain_run(built):
    g = synth.make_genome(15, [400000, 150000])
    rs = synth.make_reads(16, g, 8, 50, invalid_frac=0.25)
    assert rs.n_pairs == 400
    d = tempfile.mkdtemp(prefix="arx_e2e_bgzf_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    api.index_build(fa, fa)
    f1, f2 = os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq")
    synth.write_fastq_fast(rs, f1, f2)
    z = []
    for k, f in enumerate((f1, f2)):
        z.append(f + ".gz")
        raw = bgzfio.write_bgzf_file(z[-1], open(f, "rb").read(), cut=20000 + 3000 * k, level=4)
        assert len(bgzfio.split(raw)) >= 4
    ref = api.Reference(fa)
    try:
        # one worker: the order of the super-batches, and with it of the records in the file, is the input's in both runs
        kw = dict(pairs_per_batch=60, bam_threads=2, rec_threads=2, feeder="device", chunk_bytes=16384)
        plain = e2e.run(ref, [(f1, f2)], os.path.join(d, "plain"), workers=1, **kw)
        dev = e2e.run(ref, [tuple(z)], os.path.join(d, "bgzf"), workers=1, inflate="device", **kw)
        assert dev["pairs"] == plain["pairs"] == 400 and dev["records"] == plain["records"] and dev["batches"] == plain["batches"] >= 4
        assert dev["feeder"]["device_blocks"] == sum(len(bgzfio.split(open(p, "rb").read())) for p in z)
        assert dev["feeder"]["compressed_bytes"] == sum(os.path.getsize(p) for p in z) and plain["feeder"]["device_blocks"] == 0
        assert dev["feeder"]["bytes"] == plain["feeder"]["bytes"] == os.path.getsize(f1) + os.path.getsize(f2)
        assert bgzfio.inflate(open(os.path.join(d, "bgzf.0.bam"), "rb").read()) == bgzfio.inflate(open(os.path.join(d, "plain.0.bam"), "rb").read())
        # and with two workers, whose files together hold the same records
        two = e2e.run(ref, [tuple(z)], os.path.join(d, "two"), workers=2, inflate="device", **kw)
        a = sorted(devfeed.bam_records(os.path.join(d, "plain.0.bam")))
        b = sorted(r for k in range(2) for r in devfeed.bam_records(os.path.join(d, f"two.{k}.bam")))
        assert two["pairs"] == 400 and len(a) == 800 and a == b
        with pytest.raises(ValueError, match="feeder='device'"):
            e2e.run(ref, [tuple(z)], os.path.join(d, "no"), feeder="host", inflate="device")
    finally:
        ref.close()

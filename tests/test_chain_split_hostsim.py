"""CPU test of the split chaining (Pipeline::stage_chain with ARX_CHAIN_SPLIT=1) through the host double (tests/hostsim), which compiles the
same pipeline.h: KChainClass lists the heavy and the mid reads from occ_off alone and writes one byte per read saying who chains it, then
KChainLight, KChainMid and the heavy launch each chain their own reads.

400 reads of test_launch_paths_gpu.py's recipe (its genome, two barcodes of 100 pairs) with ARX_CHAIN_MID_MIN=1 and the heavy kernels'
thresholds lowered (12 / 3 / 6): every read with 1 .. 11 occurrences, or more than 832, asks for a place on the mid list, which holds
R / 4 + 64 = 164 -- asserted from the restatement to be fewer than ask.  A read the full list turns away is nobody's: the light launch
chains it, as KChain chained it where it found it.  The double has one stream's worth of order, so the split's launches run one after the
other there (Pipeline::fork); tests/test_side_stream_gpu.py runs them side by side.

  * the classification bytes name every read exactly once: who = heavy exactly for the reads on the heavy list, each once; who = mid exactly
    for the reads on the filled part of the mid list, each once; every other read is the light launch's; and each list holds the reads its
    rule names (restated here from the restatement's occurrence counts);
  * the chains of every read equal the restatement's, and the final results too; the unsplit double gives the same bytes.
"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import parity
import workloads
from arachne_amd import api

SIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "libarx_hostsim.so")
HEAVY_MIN, CHAIN_LDS_OCC = 12, 832
ENV = {"ARX_SIM_CHAIN_HEAVY": "1", "ARX_SIM_DEDUP_HEAVY": "1", "ARX_SIM_RESCUE_HEAVY": "1", "ARX_CHAIN_HEAVY_MIN": str(HEAVY_MIN), "ARX_DEDUP_HEAVY_MIN": "3",
       "ARX_RESCUE_HEAVY_MIN": "6", "ARX_CHAIN_MID_MIN": "1"}


def occurrences(o, seq):
    """Seed occurrences of one read as mem_chain takes them from its intervals (bwamem.c:271-276): at most max_occ = 500 per interval, evenly
    stepped; an interval is (k, l, size, begin << 32 | end)."""
    total = 0
    for s in o.collect_intv(seq)[:, 2].astype(np.int64):
        step = max(int(s) // 500, 1)
        total += min(-(-int(s) // step), 500)
    return total


@pytest.fixture(scope="module")
def env(built):
    import oradrv
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    g = workloads.nasty_genome(21, contig_lens=(200000, 120000, 50000), alt_contigs=2)
    rs = workloads.nasty_reads(21, g, n_barcodes=2, pairs_per_barcode=100)
    flat, lens = rs.seqs.reshape(-1), rs.lens
    assert rs.seqs.shape == (400, 150)
    d = tempfile.mkdtemp(prefix="arx_chain_split_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    g.write_alt(fa + ".alt")
    api.index_build(fa, fa, lib_path=SIM)
    o = oradrv.Oracle(fa)
    occ = np.array([occurrences(o, s) for s in rs.seqs])
    yield fa, o, flat, lens, occ, o.batch(flat, lens, n_threads=8)
    o.close()


def _run(fa, o, flat, lens, restated, monkeypatch, split):
    for k, v in ENV.items():
        monkeypatch.setenv(k, v)
    if split:
        monkeypatch.setenv("ARX_CHAIN_SPLIT", "1")
    else:
        monkeypatch.delenv("ARX_CHAIN_SPLIT", raising=False)
    ref = api.Reference(fa, lib_path=SIM)
    try:
        b = ref.batch(flat, lens)
        b.run(api.STAGE_CHAIN)
        klass = b.debug_chain_class() if split else None
        if not split:
            with pytest.raises(api.ArachneError, match="error %d: .*ran unsplit" % api.ARX_E_ARG):
                b.debug_chain_class()          # the stage ran unsplit: ARX_E_ARG, there is no classification to report
        b.run()
        parity.check_chains(b, o, flat, lens)
        parity.check_core(b, o, flat, lens)
        dev = b.fetch()
        parity.check_final(dev, restated)
        b.free()
        return klass, [dev[k].tobytes() for k in ("reg_off", "regs", "alns", "cigars")]
    finally:
        ref.close()


def test_split_names_every_read_once_and_chains_as_the_restatement(env, monkeypatch):
    fa, o, flat, lens, occ, restated = env
    R = len(lens)
    cap = R // 4 + 64
    heavy_want = np.flatnonzero((occ >= HEAVY_MIN) & (occ <= CHAIN_LDS_OCC))
    asks = np.flatnonzero((occ >= 1) & ~((occ >= HEAVY_MIN) & (occ <= CHAIN_LDS_OCC)))
    print(f"\nchain split: {R} reads, {len(heavy_want)} heavy, {len(asks)} ask for one of {cap} places on the mid list, {int((occ > CHAIN_LDS_OCC).sum())} above the cap")
    assert cap == 164 and len(asks) > cap and len(heavy_want) >= 30 and (occ == 0).sum() >= 1
    (who, heavy, mid, asked, mid_cap), split_bytes = _run(fa, o, flat, lens, restated, monkeypatch, True)
    assert mid_cap == cap and asked == len(asks) and len(mid) == cap
    assert sorted(heavy.tolist()) == heavy_want.tolist()                     # each once, and no other
    assert len(set(mid.tolist())) == len(mid) and set(mid.tolist()) <= set(asks.tolist())
    want = np.zeros(R, dtype=np.uint8)
    want[heavy] = 1
    want[mid] = 2
    assert (who == want).all(), np.flatnonzero(who != want)[:10]
    assert int((who == 0).sum()) == R - len(heavy_want) - cap                  # the reads turned away and the reads without a seed
    _, plain_bytes = _run(fa, o, flat, lens, restated, monkeypatch, False)
    assert split_bytes == plain_bytes

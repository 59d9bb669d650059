#!/usr/bin/env python3
"""Randomised parity sweep on the GPU: fresh seeded workloads of both generators, whole path + RFA against the CPU restatement (and
the compiled reference when it travelled), and the SMEM intervals of a sample of each seed's reads (a lost or extra SMEM often leaves the
final alignment as it was).  Not part of the test suite: a wider net cast once in a while.

usage: gpu_fuzz.py [n_seeds [first_seed [mixed|repeats|long]]] [--seed-knobs]
--seed-knobs: every seed draws the seeding kernels' knobs at random (backward-sweep kernel, bins, hand-off budget, text mode's tail,
chunk / batch / grant sizes, blocks per CU, read groups, index tables) -- tests/test_seed_variants_gpu.py walks them one by one."""
import os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from arachne_amd import api, synth
import oradrv, parity, refdrv, rfadrv, workloads

seed_knobs = "--seed-knobs" in sys.argv
argv = [a for a in sys.argv if not a.startswith("--")]
n_seeds = int(argv[1]) if len(argv) > 1 else 8
bad = 0
base = int(argv[2]) if len(argv) > 2 else 100
mode = argv[3] if len(argv) > 3 else "mixed"   # "repeats": every seed a high-copy family (long region lists, ties): the wavefront-per-item kernels
SEED_KNOBS = {   # values each knob's code supports (hip_rt.h, pipeline.h, api_impl.h); None = leave the default
    "ARX_SEED_BWD2": (None, 0, 1, 2, 3), "ARX_SEED_FIT32": (None, 0), "ARX_TEXT_BWD": (None, 0), "ARX_SEED_BWD_MID": (None, 16, 18, 21),
    "ARX_SEED_BWD_BUDGET": (None, 0, 8, 64), "ARX_SEED_BPC": (None, 1, 4), "ARX_SEED_BWD_BPC": (None, 1, 8), "ARX_STRAT_BPC": (None, 1, 8),
    "ARX_SEED_CHUNK": (None, 1, 7, 32), "ARX_SEED_BATCH": (None, 1, 16, 64), "ARX_SEED_GRANT": (None, 1, 16, 64), "ARX_SEED_GROUP": (None, 500, 1000),
    "ARX_TEXT_INDEX": (None, 0), "ARX_SA_DENSE": (None, 1, 8, 32), "ARX_KMER_K": (None, 0, 4, 12), "ARX_KMER_FWD": (None, 0),
}
for seed in range(base, base + n_seeds):
    t = time.time()
    knobs = {}
    if seed_knobs:
        kr = np.random.default_rng(9000 + seed)
        for k, vals in SEED_KNOBS.items():
            os.environ.pop(k, None)
            v = vals[int(kr.integers(0, len(vals)))] if kr.random() < 0.5 else None
            if v is not None:
                os.environ[k] = str(v); knobs[k[4:]] = v
    if mode == "repeats":
        r = np.random.default_rng(seed)
        fams = [(int(r.integers(30, 220)), int(r.integers(800, 6000)), float(r.choice([0.0, 0.002, 0.01, 0.03]))), (int(r.integers(10, 60)), int(r.integers(200, 1500)), float(r.choice([0.0, 0.05])))]
        g = synth.make_genome(seed, [int(r.integers(500_000, 2_500_000)), 50000], repeat_families=fams, n_runs=int(r.integers(0, 3)))
        rs = synth.make_reads(seed + 1, g, 5, 240, molecule_len=int(r.integers(4000, 30000)), molecules_per_barcode=int(r.integers(3, 8)))
    elif mode == "long":   # read lengths around the switch of ksw_align2's element size (250 bases), ragged, a third of the reads damaged
        r = np.random.default_rng(seed)
        L = int(r.choice([255, 252, 250, 249, 230]))
        g = synth.make_genome(seed, [int(r.integers(300_000, 1_500_000)), 60000], repeat_families=[(int(r.integers(5, 40)), int(r.integers(300, 2000)), 0.01)])
        rs = synth.make_reads(seed + 1, g, 4, 220, read_len=L, sub_rate=0.01)
        for i in r.choice(rs.seqs.shape[0], size=rs.seqs.shape[0] // 3, replace=False):
            m = r.random(L) < (0.1, 0.2, 0.35)[i % 3]
            rs.seqs[i, m] = r.integers(0, 4, size=int(m.sum()), dtype=np.uint8)
        if seed % 2:
            rs.lens[r.choice(len(rs.lens), size=len(rs.lens) // 4, replace=False)] = r.integers(30, L + 1, size=len(rs.lens) // 4)
    elif seed % 3 == 0:
        g = synth.make_genome(seed, [1500000, 400000]); rs = synth.make_reads(seed + 1, g, 6, 500)
    else:
        g = workloads.nasty_genome(seed, contig_lens=(180000 + 1000 * (seed % 7), 90000, 40000), alt_contigs=seed % 3)
        rs = workloads.nasty_reads(seed, g, n_barcodes=6, pairs_per_barcode=400)
    d = tempfile.mkdtemp(prefix="arx_fuzz_"); fa = os.path.join(d, "g.fa")
    g.write_fasta(fa); g.write_alt(fa + ".alt")
    api.index_build(fa, fa)
    po = rs.pair_offsets()
    rng = np.random.default_rng(7000 + seed)   # PCR duplicates and unmappable pairs inside every barcode (markDuplicates)
    for bi in range(len(po) - 1):
        lo, hi = int(po[bi]), int(po[bi + 1])
        for _ in range((hi - lo) // 20):
            i, j = rng.integers(lo, hi, size=2)
            rs.seqs[2 * j:2 * j + 2] = rs.seqs[2 * i:2 * i + 2]; rs.lens[2 * j:2 * j + 2] = rs.lens[2 * i:2 * i + 2]
        for j in rng.integers(lo, hi, size=3):
            rs.seqs[2 * j:2 * j + 2] = rng.integers(0, 4, size=rs.seqs[2 * j:2 * j + 2].shape)
    ref = api.load_reference(fa, 0)
    o = oradrv.Oracle(fa)
    S = rs.seqs if (rs.lens == rs.seqs.shape[1]).all() else np.concatenate([rs.seqs[i, :rs.lens[i]] for i in range(len(rs.lens))])   # ragged: flat
    try:
        b = ref.batch(S, rs.lens).run()
        sample = np.random.default_rng(8000 + seed).choice(len(rs.lens), size=min(300, len(rs.lens)), replace=False)
        parity.check_intervals(b, o, S, rs.lens, reads=sorted(sample.tolist()))
        dev = b.fetch()
        ora = o.batch(S, rs.lens, n_threads=8)
        parity.check_final(dev, ora)
        if refdrv.available():
            r = refdrv.Ref(fa); parity.check_final(dev, r.batch(S, rs.lens, n_threads=8))
        po = rs.pair_offsets()
        flags = [rfadrv.worth_running_rfa(rs.barcodes[i], int(po[i + 1] - po[i])) for i in range(len(po) - 1)]
        names, offs, clens, alt, l_pac = ref.contigs()
        orfa = rfadrv.oracle_rfa(ora, rs.lens, po, flags, l_pac, offs)
        parity.check_rfa(b.rfa(po, flags), orfa)
        parity.check_post(b.post(), rfadrv.oracle_post(o.h, ora, S, rs.lens, po, offs, orfa))
        print("seed %d ok: %d regions, intervals of %d reads, %.1fs%s" % (seed, len(dev["regs"]), len(sample), time.time() - t, (" knobs %s" % knobs) if seed_knobs else ""), flush=True)
    except AssertionError as e:
        bad += 1
        print("seed %d MISMATCH%s: %s" % (seed, (" knobs %s" % knobs) if seed_knobs else "", str(e)[:300]), flush=True)
    ref.close(); o.close()
print("fuzz done, %d mismatching seeds" % bad)
sys.exit(1 if bad else 0)

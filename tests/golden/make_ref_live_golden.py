"""Generates tests/golden/ref_live_v1.npz and ref_nasty<seed>_v1.npz from the reference's own C core (oracle/_ref/libbwaref.so, compiled in place by
oracle/Makefile).  Runs only where the reference's sources exist.

The fixture is DATA: what the reference computed for the seeded inputs of the tests that compare against it live, so that they
still compare against it where oracle/_ref cannot be built:
  - index_<lens>_{fasta,bwt,sa,pac,ann,amb}: sha256 of the genome FASTA and of the files its `bwa index` path wrote, for the fresh
    genomes of test_index_build.py (FRESH_LENS) and test_index_build_gpu.py (gpuidx_<case>_*);
  - ksw_live: ksw_align2's results for the calls of test_ksw_i16.py's live comparison, in order;
  - pair<seed>_{reg_off,regs,alns,cigars} and pair<seed>_idx_<ext>: the per-pair path (regions, alignment records, CIGARs) and the
    index digests for the nasty workloads of test_oracle_vs_ref.py;
and tests/golden/ref_nasty<seed>_v1.npz: nasty<seed>_* the same for test_gpu_parity.py's nasty workloads.

usage: python tests/golden/make_ref_live_golden.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import refdrv  # noqa: E402
import test_gpu_parity  # noqa: E402
import test_index_build  # noqa: E402
import test_index_build_gpu  # noqa: E402
import test_ksw_i16  # noqa: E402
import test_oracle_vs_ref  # noqa: E402
import workloads  # noqa: E402

EXTS = test_index_build.INDEX_EXTS


def index_digests(out, key, g, with_alt=False):
    d = tempfile.mkdtemp(prefix="arx_reflive_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    if with_alt:
        g.write_alt(fa + ".alt")
    out[key + "_fasta"] = np.array(test_index_build.sha256(fa))
    assert refdrv.Ref().index_build(fa, fa) == 0
    for ext in EXTS:
        out[key + "_" + ext] = np.array(test_index_build.sha256(fa + "." + ext))
    return fa


def pair_path(out, key, g, rs, threads):
    fa = index_digests(out, key + "_idx", g, with_alt=True)
    r = refdrv.Ref()
    r.open(fa)
    res = r.batch(rs.seqs, rs.lens, n_threads=threads)
    for k in test_oracle_vs_ref.KEYS:
        a = res[k]
        if a.dtype == np.int64:              # stored as 32-bit integers (the tests widen them again); nothing here needs more
            assert np.abs(a).max(initial=0) < 2 ** 31, k
            a = a.astype(np.int32)
        out[key + "_" + k] = a
    r.close()


def main():
    assert refdrv.available(), "oracle/_ref/libbwaref.so missing: make -C oracle ref"
    out = {}
    for lens in test_index_build.FRESH_LENS:
        fa = index_digests(out, "index_" + "x".join(map(str, lens)), test_index_build.fresh_genome(lens))
    for case in test_index_build_gpu.GENOME_CASES:
        index_digests(out, "gpuidx_" + case, test_index_build_gpu.case_genome(case))
    r = refdrv.Ref(fa)          # ksw_align2 takes its scoring from an opened index (any of them: the calls do not read the index)
    out["ksw_live"] = np.stack([r.ksw_align2(q, t, x) for _it, q, t, x in test_ksw_i16.live_cases()])
    r.close()
    for seed in (1, 2):
        g, rs = test_oracle_vs_ref.pair_path_inputs(seed)
        pair_path(out, "pair%d" % seed, g, rs, 2)
    files = [("ref_live_v1.npz", out)]
    for seed in test_gpu_parity.NASTY_SEEDS:         # one file per workload: each stays well below 1 MiB
        g, rs = test_gpu_parity.nasty_inputs(seed)
        nasty = {}
        pair_path(nasty, "nasty%d" % seed, g, rs, 8)
        files.append(("ref_nasty%d_v1.npz" % seed, nasty))
    for name, arrays in files:
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""CPU test of the seeding stage on the seed_shapes workload (tests/workloads.py), through the host double (tests/hostsim).

Two things are pinned here.
  * The INPUT: the restatement's shape entry (ora_seed_shapes: one row per bwt_smem1a call and third-pass start) says what the reads make a
    seeding kernel do, and the conditions below -- list lengths on either side of every bin edge with the start inside the read, rows wider
    than one and two 64-entry chunks, sweeps tens of rows deep and far above the hand-off budget, text mode's triggers met and not met, the
    table jumps taken and refused in every pass -- are asserted from it alone, never from the code under test.  tests/test_seed_variants_gpu.py
    runs the same reads through every kernel variant on the GPU; without these conditions its equalities would say little.
  * The double: intervals (STAGE_SEED) and chains (STAGE_CHAIN) of EVERY read equal the restatement's for each open-time variant the double
    honours.
"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import seedcheck
import workloads
from arachne_amd import api

SIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "libarx_hostsim.so")


@pytest.fixture(scope="module")
def env(built):
    import oradrv
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    g, flat, lens, kinds = workloads.seed_shapes()
    d = tempfile.mkdtemp(prefix="arx_seed_shapes_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    api.index_build(fa, fa, lib_path=SIM)
    o = oradrv.Oracle(fa)
    ref = api.Reference(fa, lib_path=SIM)
    info = ref.index_info()
    ref.close()
    exp = seedcheck.Expected(o, flat, lens, kf=info["kmer_fwd_depth"], k3=info["kmer_k"] > 0)
    yield fa, o, flat, lens, kinds, exp
    o.close()


def test_shape_entry_replays_collect_intv(env):
    """The shape entry's intervals come from the run its rows describe: they are ora_collect_intv's, read by read."""
    fa, o, flat, lens, kinds, exp = env
    n = 0
    for r in range(len(lens)):
        if lens[r] < 19:
            continue
        want = o.collect_intv(exp.flat[exp.off[r]:exp.off[r + 1]])
        assert exp.n[r] == len(want) and (exp.iv[r, :len(want)] == want).all(), r
        n += len(want)
    assert n == int(exp.n.sum()) and n > 10000


def test_workload_reaches_the_rare_paths(env):
    fa, o, flat, lens, kinds, exp = env
    cov = exp.coverage()
    print("\nseed_shapes:", len(lens), "reads,", {k: len(v) for k, v in kinds.items()}, "lengths", int(lens.min()), "..", int(lens.max()))
    print({k: (v if not isinstance(v, set) else f"{len(v)} distinct, max {max(v)}") for k, v in cov.items()})
    print("census the GPU must report:", exp.census())
    assert lens.max() == 255 and {18, 19, 20} <= set(lens.tolist())
    # either side of every bin edge (16 | 17, 21 | 22, 32 | 33, 64 | 65) and of two 64-entry chunks, with the start inside the read
    missing = [v for v in seedcheck.EDGE_LENGTHS if v not in cov["list_lengths_swept"]]
    assert not missing, missing
    assert max(cov["list_lengths_swept"]) >= 193            # four chunks in k_seed_bwd_wave
    later = exp.col("widest")[(exp.col("pass") < 3) & (exp.col("x") > 0)]
    assert (later >= 65).any() and (later >= 129).any()
    assert cov["most_rows_above_16"] >= 30
    assert cov["sweeps_above_128_ext"] >= 50
    assert cov["fwd_text"] >= 50 and cov["fwd_no_text"] >= 50
    assert cov["sweep_text"] >= 50 and cov["sweep_no_text"] >= 50
    # the table jumps (oradrv.Oracle.JUMP_*): taken and refused at least 20 times in each pass.  The reasons a pass can meet: an ambiguous base or
    # the end of the read in front of the jump (first and third pass; a re-seeding start lies in the middle of a match of at least 28 bases, so
    # the 14 bases a table can hold are inside it), a k-mer rarer than min_intv (first pass: one that does not occur; re-seeding; the third pass
    # has no such test)
    for ps in (1, 2, 3):
        j = cov[f"jump{ps}"]
        assert j[-1] == 0 and j[0] >= 20 and j[1] + j[2] + j[3] >= 20, (ps, j)
    assert min(cov["jump1"][k] for k in (1, 2, 3)) >= 20, cov["jump1"]
    assert cov["jump2"][3] >= 20 and cov["jump2"][1] == 0 and cov["jump2"][2] == 0, cov["jump2"]
    assert min(cov["jump3"][k] for k in (1, 2)) >= 20 and cov["jump3"][3] == 0, cov["jump3"]
    # exact copies: intervals above max_occ = 500 and on either side of max_mem_intv = 20; re-seeding (min_intv > 1) from long seeds
    s = exp.iv[:, :, 2][np.arange(api.CAP_INTV)[None, :] < exp.n[:, None]]
    assert (s > 500).sum() >= 20 and ((s >= 20) & (s <= 30)).sum() >= 20 and ((s > 10) & (s < 20)).sum() >= 20
    assert len(set(exp.col("min_intv")[exp.col("pass") == 2].tolist())) >= 8
    assert exp.n.max() >= 20 and exp.n.max() <= api.CAP_INTV


def test_capped_variant_still_has_long_lists():
    """The batch cut to 150 bases (the seeding kernels' LDS row shrinks with the longest read): same reads, shorter."""
    g, flat, lens, kinds = workloads.seed_shapes(cap=150)
    g2, flat2, lens2, kinds2 = workloads.seed_shapes()
    assert lens.max() == 150 and len(lens) == len(lens2) and (lens == np.minimum(lens2, 150)).all()
    off, off2 = np.concatenate([[0], np.cumsum(lens)]), np.concatenate([[0], np.cumsum(lens2)])
    for r in (0, 1, len(lens) // 2, len(lens) - 1):
        assert (flat[off[r]:off[r + 1]] == flat2[off2[r]:off2[r] + lens[r]]).all()


OPEN_VARIANTS = [
    {},
    {"ARX_TEXT_INDEX": "0"},
    {"ARX_KMER_K": "0"},
    {"ARX_KMER_K": "4"},
    {"ARX_KMER_K": "14"},                               # (the double's memory rule stops at 13)
    {"ARX_KMER_FWD": "0"},
    {"ARX_KMER_K": "4", "ARX_TEXT_INDEX": "0"},
    {"ARX_SEED_GROUP": "700"},                          # three passes through a group-sized pool, the last one short
    {"ARX_SEED_BWD_ENTRY": "1"},                        # the double's entry-by-entry sweep: what k_seed_bwd_e rests on
    {"ARX_SEED_BWD_ENTRY": "1", "ARX_TEXT_INDEX": "0"},
]


@pytest.mark.parametrize("var", OPEN_VARIANTS, ids=lambda v: ",".join(f"{k[4:]}={x}" for k, x in v.items()) or "default")
def test_every_read_matches_restatement(env, monkeypatch, var):
    fa, o, flat, lens, kinds, exp = env
    for k, v in var.items():
        monkeypatch.setenv(k, v)
    ref = api.Reference(fa, lib_path=SIM)
    try:
        info = ref.index_info()
        assert info["text_mode"] == (var.get("ARX_TEXT_INDEX") != "0")
        want_k = int(var.get("ARX_KMER_K", 10))
        assert info["kmer_k"] == min(want_k, 13), info
        assert info["kmer_fwd_depth"] == (0 if var.get("ARX_KMER_FWD") == "0" else info["kmer_k"])
        b = ref.batch(flat, lens)
        b.seed_census(True)
        b.run(api.STAGE_SEED)
        n_iv = exp.check_intervals(b, str(var))
        b.run(api.STAGE_CHAIN)
        n_ch = exp.check_chains(b, str(var))
        cen = b.seed_census()
        assert not any(cen.values()), cen       # the double has no bins, hand-offs or tails: the entry exists and reports zeros
        print(f"\n{var or 'default'}: {len(lens)} reads, {n_iv} intervals, {n_ch} chains equal the restatement's; index {info}")
        b.free()
    finally:
        ref.close()

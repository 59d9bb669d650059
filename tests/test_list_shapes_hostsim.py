"""CPU test of the list stages (chaining and chain filter, region de-duplication, mate rescue) on the list_shapes workload (tests/workloads.py),
through the host double (tests/hostsim).

Two things are pinned here.
  * The INPUT: the restatement's shape entry (ora_list_shapes: counts taken inside mem_chain, mem_chain_flt, mem_sort_dedup_patch,
    mem_patch_reg and mem_matesw) says what the reads make a list kernel do, and the conditions below -- list lengths on either side of
    every 64-lane step, of the 256-entry sorts and guards and of every LDS class, the kept rank that decides a drop, redundant regions across
    a 64-entry word, insertions at either end of long mate lists, ties -- are asserted from it alone, never from the code under test.
    tests/test_wave_lists_gpu.py runs the same pairs through every variant of the wavefront-per-item kernels (k_chain_heavy, k_dedup_heavy,
    k_rescue_heavy: code that exists on the GPU only); without these conditions its equalities would say little.
  * The double: chains, core regions and final results of EVERY read equal the restatement's, with the heavy items listed and handed over
    (the double runs the serial code on them) and without.

Two conditions stay printed, not asserted, because no planted input reaches them in a read's own pass:
  * mem_patch_reg reaching its alignment in a list of 65 .. 256 regions (the -2 hand-back of k_dedup_heavy): its ratio test lets only gaps
    through that the extension crosses anyway; tests/test_config_shapes.py keeps that path at short lists;
  * the final sort of mem_sort_dedup_patch dropping an identical (score, rb, qb) neighbour: two such regions overlap entirely, so the
    redundancy loop, which runs first and scans every neighbour within max_chain_gap, has always removed one of them.
"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import listshapes
import parity
import workloads
from arachne_amd import api

SIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "libarx_hostsim.so")


@pytest.fixture(scope="module")
def env(built):
    import oradrv
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    g, flat, lens, kinds = workloads.list_shapes()
    d = tempfile.mkdtemp(prefix="arx_list_shapes_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    g.write_alt(fa + ".alt")
    api.index_build(fa, fa, lib_path=SIM)
    o = oradrv.Oracle(fa)
    sh = listshapes.Shapes(o, flat, lens)
    yield fa, o, g, flat, lens, kinds, sh
    o.close()


def _at_least_two(sh, name, values):
    missing = [v for v in values if sh.count(name, v) < 2]
    assert not missing, (name, missing)


def test_workload_is_small(env):
    fa, o, g, flat, lens, kinds, sh = env
    assert g.total_len <= 650_000 and len(lens) <= 400 and len(lens) % 2 == 0 and lens.max() <= 255


def test_workload_reaches_the_list_edges(env):
    fa, o, g, flat, lens, kinds, sh = env
    occ, built, srt, kept, regs = (sh.col(k) for k in ("occ", "built", "sorted", "kept", "regs_in"))
    print("\nlist_shapes:", len(lens), "reads,", {k: len(v) for k, v in kinds.items()}, "genome", g.total_len)
    print("occurrences", sorted(set(occ[occ >= 31].tolist())))
    print("regions before the pass", sorted(set(regs[regs >= 31].tolist())))
    # ---- seed occurrences: either side of the 64-lane steps, of CHAIN_LDS_SMALL and of CHAIN_LDS_OCC; beyond it a read that still has many chains
    _at_least_two(sh, "occ", [63, 64, 65, 127, 128, 129, 255, 256, 257, 831, 832, 833])
    assert ((occ > 832) & (built > 64)).sum() >= 1
    # ---- chains built (= the chains the filter sorts: 256 | 257 are the two w_introsort instances)
    _at_least_two(sh, "built", [64, 65, 128, 129, 256, 257])
    _at_least_two(sh, "sorted", [256, 257])
    # ---- chains kept: a chain dropped with 65+ and 129+ kept ones in front of it; drops decided by the kept chain of rank 62, 63 (lane 63 of the
    # filter's first step) and 64 (lane 0 of its second)
    kad = sh.col("kept_at_drop")
    assert (kad >= 65).sum() >= 2 and (kad >= 129).sum() >= 2
    for k in ("drop62", "drop63", "drop64"):
        assert (sh.col(k) >= 1).sum() >= 2, k
    assert ((srt > 64) & (sh.col("w_run") >= 3)).sum() >= 3
    # ---- regions before mem_sort_dedup_patch
    _at_least_two(sh, "regs_in", [31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257])
    far, stopped_far = sh.col("redun_far"), sh.col("stopped_far")
    long_lists = regs >= 65
    print("redundancy loop: lists with removals", int((sh.col("redun") > 0).sum()), "| removed entry >= 64 and stopper in another word:", int((far > 0).sum()),
          "| the later entry goes, stopper in another word:", int((stopped_far > 0).sum()))
    assert ((far > 0) & (regs <= 256)).sum() >= 2          # (in lists k_dedup_heavy takes)
    assert ((stopped_far > 0) & (regs <= 256)).sum() >= 1
    print("final sort: identical neighbours dropped in", int((sh.col("ident") > 0).sum()), "lists, across a 64 boundary in", int((sh.col("ident_far") > 0).sum()))
    print("mem_patch_reg reaches its alignment in", int(((sh.col("patch_aln") > 0) & long_lists & (regs <= 256)).sum()), "lists of 65 .. 256 regions, merges in",
          int(((sh.col("patch_merged") > 0) & long_lists & (regs <= 256)).sum()))
    # ---- rescue: the mate list's length before an insertion
    ln, pos, tie, removed = (sh.icol(k) for k in ("len", "pos", "tie", "removed"))
    print("insertions:", len(ln), "into lists of", sorted(set(ln.tolist())))
    missing = [v for v in (63, 64, 65, 127, 128, 255, 256, 257) if (ln == v).sum() < 2]
    assert not missing, missing
    assert (ln >= 258).sum() >= 2
    long_ = ln >= 64
    assert (long_ & (pos == 0)).sum() >= 1 and (long_ & (pos == ln)).sum() >= 2 and (long_ & (removed > 0)).sum() >= 2
    assert ((ln >= 65) & (tie == 1)).sum() >= 2
    assert ((ln >= 64) & (ln <= 256) & (tie == 0) & (removed > 0)).sum() >= 2       # (w_dedup_insert settles these itself)
    print("insertions with two equal-ended stoppers in different 64-entry steps (w_dedup_insert's choice between them):", int((sh.icol("stoppers_far") > 0).sum()))
    # ---- pairs by the sums of their core lists and of their capacities (KPairCap, restated in listshapes.pair_cap)
    core, cap = sh.caps()
    for v in (170, 171, 340, 341, 680, 681):
        assert (cap == v).sum() >= 2, v
    for v in (47, 48):
        assert (core == v).sum() >= 2, v
    assert not ((cap == 681) & (core < 48)).any()           # 681 is kept from the heavy kernel by its capacity alone
    print("census the GPU must report by default:", sh.census(), "| with lowered thresholds:", sh.census(12, 3, 6))


VARIANTS = [
    {},
    {"ARX_SIM_CHAIN_HEAVY": "1", "ARX_SIM_DEDUP_HEAVY": "1", "ARX_SIM_RESCUE_HEAVY": "1", "ARX_CHAIN_HEAVY_MIN": "12", "ARX_DEDUP_HEAVY_MIN": "3", "ARX_RESCUE_HEAVY_MIN": "6"},
]


@pytest.fixture(scope="module")
def restated(env):
    fa, o, g, flat, lens, kinds, sh = env
    return o.batch(flat, lens, n_threads=8)


@pytest.mark.parametrize("var", VARIANTS, ids=["default", "heavy lists, lowered thresholds"])
def test_every_read_matches_restatement(env, restated, monkeypatch, var):
    fa, o, g, flat, lens, kinds, sh = env
    for k, v in var.items():
        monkeypatch.setenv(k, v)
    ref = api.Reference(fa, lib_path=SIM)
    try:
        b = ref.batch(flat, lens)
        b.heavy_census(True)
        b.run()
        parity.check_chains(b, o, flat, lens)
        parity.check_core(b, o, flat, lens)
        parity.check_final(b.fetch(), restated)
        cen = b.heavy_census()
        assert not any(cen.values()), cen       # the double keeps no census: the entry exists and reports zeros
        b.free()
    finally:
        ref.close()

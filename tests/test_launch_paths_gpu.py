"""The host-side launch choices that no batch-level test exercises, each on the GPU against the restatement (-m gpu).

Which kernel the runtime starts for a stage, with what grid and on which stream, is decided on the host by per-batch switches
(arachne_amd/csrc/switches.h): the capped or uncapped item launch, the side stream, merged or per-class extension launches, the older
extension kernel, the one-thread rescue SW, the SW prefilter, the rescue replay's LDS classes, the one-lane forms of the heavy kernels, the
16-lane chaining groups, the small placement workgroups, one resident block per CU (every capped launch grid-strides), the backward-sweep
variants, and locate without the whole suffix array.  Every case runs the same 1,000 reads with the heavy kernels' thresholds lowered so that
every heavy list and the mid list is non-empty -- asserted from the restatement's stage outputs before the device is looked at -- and must
give the restatement's final regions, alignment records and CIGARs (parity.check_final) and placed candidates (parity.check_rfa) bit for
bit.  The restatement runs once.

Launch census: per case, the map launch name -> (calls, items) of Reference.kernel_times() equals tests/golden/launch_census_v1.json, which
tests/golden/make_launch_census.py records on the GPU from a build of the commit BEFORE the launch layer (csrc/hip_launch.h) through
run_case() below, twice, and writes only if both recordings agree.  Every value is a host-side count of deterministic quantities; times are
not compared.
"""
import json
import os
import tempfile

import numpy as np
import pytest

import parity
import rfadrv
import workloads
from arachne_amd import api

pytestmark = pytest.mark.gpu

CENSUS = os.path.join(workloads.GOLDEN_DIR, "launch_census_v1.json")
THRESHOLDS = {"ARX_CHAIN_HEAVY_MIN": 12, "ARX_DEDUP_HEAVY_MIN": 3, "ARX_RESCUE_HEAVY_MIN": 6}   # test_heavy_item_split_hostsim's
CASES = [
    {},
    {"ARX_WIDE": 0},
    {"ARX_AUX_STREAM": 1},
    {"ARX_EXT_MERGE": 0},                   # always per-class launches
    {"ARX_EXT_MERGE": 2000000000},          # always merged
    {"ARX_EXT_OLD": 1},
    {"ARX_SW_SIMPLE": 1},
    {"ARX_SW_FILTER": 1},
    {"ARX_RESCUE_LDS_CLASSES": 1},
    {"ARX_RESCUE_WAVE": 0},
    {"ARX_CHAIN_WAVE": 0},
    {"ARX_CHAIN_GROUP": 1},
    {"ARX_RFA_SMALL": 1},
    {"ARX_BPC": 1, "ARX_COOP_BPC": 1},      # every capped launch grid-strides
    {"ARX_SEED_BWD2": 0},
    {"ARX_SEED_BWD2": 1},
    {"ARX_SEED_BWD2": 3},
    {"ARX_TEXT_INDEX": 0},                  # a context of its own: k_locate_dyn
]
KNOBS = sorted({k for c in CASES for k in c} | set(THRESHOLDS))


def label(var):
    return ",".join(f"{k[4:]}={v}" for k, v in var.items()) or "default"


def make_workload():
    g = workloads.nasty_genome(21, contig_lens=(200000, 120000, 50000), alt_contigs=2)
    rs = workloads.nasty_reads(21, g, n_barcodes=2, pairs_per_barcode=250)
    d = tempfile.mkdtemp(prefix="arx_launch_paths_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    g.write_alt(fa + ".alt")
    api.index_build(fa, fa)
    return fa, rs


def set_case_env(var, setenv, delenv):
    for k in KNOBS:
        delenv(k)
    for k, v in {**THRESHOLDS, **var}.items():
        setenv(k, str(v))


def run_case(ref, rs, flags):
    """One batch handle through the whole path with every launch counted: (final results, placed candidates, {launch name: [calls, items]}).
    The environment is the caller's business (set_case_env) and is set before this creates the handle."""
    po = rs.pair_offsets()
    ref.kernel_times_reset(True)
    b = ref.batch(rs.seqs, rs.lens)
    try:
        dev = b.run().fetch()
        cands = b.rfa(po, flags)
    finally:
        b.free()
    census = {k: [v["calls"], v["items"]] for k, v in sorted(ref.kernel_times(cap=256).items())}
    ref.kernel_times_reset(False)
    return dev, cands, census


def occurrences(o, seq):
    """Seed occurrences of one read as mem_chain takes them from its intervals (bwamem.c:271-276): at most max_occ = 500 per interval, evenly
    stepped; an interval is (k, l, size, begin << 32 | end)."""
    total = 0
    for s in o.collect_intv(seq)[:, 2].astype(np.int64):
        step = max(int(s) // 500, 1)
        total += min(-(-int(s) // step), 500)
    return total


@pytest.fixture(scope="module")
def wl(built):
    import oradrv
    fa, rs = make_workload()
    assert rs.seqs.shape == (1000, 150)
    o = oradrv.Oracle(fa)
    po = rs.pair_offsets()
    flags = [rfadrv.worth_running_rfa(rs.barcodes[i], int(po[i + 1] - po[i])) for i in range(len(po) - 1)]
    assert flags == [True, True]
    # what the workload makes the host choose between, from the restatement's stage outputs alone
    occ = np.array([occurrences(o, rs.seqs[r]) for r in range(len(rs.lens))])
    core = np.array([len(o.align1(rs.seqs[r])) for r in range(len(rs.lens))])
    ora = o.batch(rs.seqs, rs.lens, n_threads=8)
    have = dict(occ16=int((occ >= 16).sum()), occ64=int((occ >= 64).sum()), occ12to63=int(((occ >= 12) & (occ < 64)).sum()),
                core3=int((core >= 3).sum()), pair6=int((core[0::2] + core[1::2] >= 6).sum()), final=len(ora["regs"]))
    print(f"\nlaunch-path workload: {have}")
    assert min(have.values()) >= 30, have
    yield fa, rs, flags, ora
    o.close()


@pytest.fixture(scope="module")
def refs(wl):
    """One context per index form, opened when a case first asks for it."""
    fa = wl[0]
    opened = {}

    def get(text_index):
        if text_index not in opened:
            old = os.environ.pop("ARX_TEXT_INDEX", None)
            if not text_index:
                os.environ["ARX_TEXT_INDEX"] = "0"
            try:
                opened[text_index] = api.load_reference(fa, 0)
            finally:
                os.environ.pop("ARX_TEXT_INDEX", None)
                if old is not None:
                    os.environ["ARX_TEXT_INDEX"] = old
            assert opened[text_index].index_info()["text_mode"] == text_index
        return opened[text_index]
    yield get
    for r in opened.values():
        r.close()


results = {}    # label -> census of the case that ran (test_launch_census reads it; parity is asserted where the case runs)


@pytest.mark.parametrize("var", CASES, ids=[label(v) for v in CASES])
def test_launch_path_equals_restatement(wl, refs, monkeypatch, var):
    fa, rs, flags, ora = wl
    ref = refs(str(var.get("ARX_TEXT_INDEX", 1)) != "0")
    set_case_env(var, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    dev, cands, census = run_case(ref, rs, flags)
    results[label(var)] = census
    parity.check_final(dev, ora)
    names, offs, clens, alt, l_pac = ref.contigs()
    parity.check_rfa(cands, rfadrv.oracle_rfa(ora, rs.lens, rs.pair_offsets(), flags, l_pac, offs))
    assert int((cands["cands"]["active"] == 1).sum()) == len(rs.lens)      # one placement per read


@pytest.mark.parametrize("var", CASES, ids=[label(v) for v in CASES])
def test_launch_census(wl, refs, monkeypatch, var):
    """calls and items of every launch name, against the table recorded before the launch layer (a field the two recordings disagreed on is
    null in the table and not compared; calls never is)."""
    with open(CENSUS) as f:
        want = json.load(f)["cases"][label(var)]
    fa, rs, flags, ora = wl
    if label(var) not in results:       # (run alone: the parity test of the same case has not left its census)
        set_case_env(var, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
        results[label(var)] = run_case(refs(str(var.get("ARX_TEXT_INDEX", 1)) != "0"), rs, flags)[2]
    got = results[label(var)]
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    for name, (calls, items) in want.items():
        assert calls is not None and got[name][0] == calls, (name, got[name], (calls, items))
        if items is not None:
            assert got[name][1] == items, (name, got[name], (calls, items))

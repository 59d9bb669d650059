"""The wavefront-per-item list kernels (k_chain_heavy, k_dedup_heavy, k_rescue_heavy: arx_cold.hip, dev_chain_wave.h, dev_regs_wave.h) on the
list_shapes workload, every variant against the restatement on every read and pair, bit for bit (-m gpu).

The host double runs the serial code for the items these kernels take, so their lines are held only by what the GPU suite sends through
them.  tests/test_list_shapes_hostsim.py asserts from the restatement alone that this workload sits on their lane, word and LDS-class edges
(63 | 64 | 65 ... 831 | 832 | 833 seed occurrences, 256 | 257 chains, drops decided by the kept chain of rank 62 | 63 | 64, region lists of
31 .. 257 entries with redundant entries across a 64-entry word, insertions into mate lists of 63 .. 263 entries at either end, ties,
capacity sums on either side of 170 | 340 | 680).  Here every variant's chains, core regions and final results equal the restatement's,
and WHICH kernel ran is asserted, not assumed: Batch.heavy_census() (arx_batch_debug_heavy_census, off outside tests) reports the lengths of
the three heavy lists, which must equal what the restatement's shapes give for the variant's thresholds (listshapes.Shapes.census).

One index and one restatement run per module; the restatement's per-read answers are computed once and shared by the variants.
"""
import os
import tempfile
import time

import numpy as np
import pytest

import listshapes
import parity
import rfadrv
import workloads
from arachne_amd import api

pytestmark = pytest.mark.gpu

LOWERED = {"ARX_CHAIN_HEAVY_MIN": 12, "ARX_DEDUP_HEAVY_MIN": 3, "ARX_RESCUE_HEAVY_MIN": 6}     # tests/test_launch_paths_gpu.py's: lists of 2 .. 31 entries take the wave code too
VARIANTS = [
    {},
    {"ARX_CHAIN_WAVE": 0},
    {"ARX_RESCUE_WAVE": 0},
    {"ARX_DEDUP_HEAVY": 0},
    {"ARX_RESCUE_LDS_CLASSES": 1},
    {"ARX_AUX_STREAM": 1},
    dict(LOWERED),
    {"ARX_CHAIN_GROUP": 1, "ARX_CHAIN_HEAVY_MIN": 128},
]
KNOBS = sorted({k for v in VARIANTS for k in v})


def label(var):
    return ",".join(f"{k[4:]}={v}" for k, v in var.items()) or "default"


class Restated:
    """The restatement's per-read answers, computed on first use and kept (parity.check_* ask for them read by read)."""

    def __init__(self, o):
        self.o, self.c, self.a = o, {}, {}

    def chains(self, seq, do_flt):
        k = (seq.tobytes(), do_flt)
        if k not in self.c:
            self.c[k] = self.o.chains(seq, do_flt)
        return self.c[k]

    def align1(self, seq):
        k = seq.tobytes()
        if k not in self.a:
            self.a[k] = self.o.align1(seq)
        return self.a[k]


@pytest.fixture(scope="module")
def wl(built):
    import oradrv
    g, flat, lens, kinds = workloads.list_shapes()
    d = tempfile.mkdtemp(prefix="arx_wave_lists_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    g.write_alt(fa + ".alt")
    api.index_build(fa, fa)
    o = oradrv.Oracle(fa)
    sh = listshapes.Shapes(o, flat, lens)
    ora = o.batch(flat, lens, n_threads=8)
    ref = api.load_reference(fa, 0)
    t0 = time.time()
    yield dict(fa=fa, o=o, rest=Restated(o), flat=flat, lens=lens, off=np.concatenate([[0], np.cumsum(lens)]), sh=sh, ora=ora, ref=ref)
    print(f"\nwave-list variants: {time.time() - t0:.1f} s behind the module's fixture")
    ref.close()
    o.close()


def set_env(monkeypatch, var):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in var.items():
        monkeypatch.setenv(k, str(v))


def expected_census(sh, var, reads=None):
    return sh.census(chain_min=var.get("ARX_CHAIN_HEAVY_MIN", listshapes.CHAIN_HEAVY_MIN), dedup_min=var.get("ARX_DEDUP_HEAVY_MIN", listshapes.DEDUP_HEAVY_MIN),
                     rescue_min=var.get("ARX_RESCUE_HEAVY_MIN", listshapes.RESCUE_HEAVY_MIN), dedup_heavy=var.get("ARX_DEDUP_HEAVY", 1) != 0,
                     classes=var.get("ARX_RESCUE_LDS_CLASSES", 0) != 0, reads=reads)


def slice_ora(ora, r0, r1):
    """The restatement's batch result for reads r0 .. r1 (whole pairs), offsets made relative."""
    g0, g1 = int(ora["reg_off"][r0]), int(ora["reg_off"][r1])
    alns = ora["alns"][g0:g1].copy()
    c0 = int(alns[0, 8]) if g1 > g0 else 0
    c1 = int(alns[-1, 8] + alns[-1, 7]) if g1 > g0 else 0
    alns[:, 8] -= c0
    return dict(reg_off=ora["reg_off"][r0:r1 + 1] - g0, regs=ora["regs"][g0:g1], alns=alns, cigars=ora["cigars"][c0:c1])


def check_batch(w, b, var, r0=None, r1=None):
    """Chains, core regions and final results of reads r0 .. r1 of the workload (default: all) as the batch handle holds them, and its census."""
    r0 = 0 if r0 is None else r0
    r1 = len(w["lens"]) if r1 is None else r1
    flat, lens = w["flat"][w["off"][r0]:w["off"][r1]], w["lens"][r0:r1]
    parity.check_chains(b, w["rest"], flat, lens)
    parity.check_core(b, w["rest"], flat, lens)
    dev = b.fetch()
    parity.check_final(dev, slice_ora(w["ora"], r0, r1))
    return dev


@pytest.mark.parametrize("var", VARIANTS, ids=[label(v) for v in VARIANTS])
def test_variant_equals_restatement_and_census(wl, monkeypatch, var):
    w = wl
    set_env(monkeypatch, var)
    b = w["ref"].batch(w["flat"], w["lens"])
    try:
        b.heavy_census(True)
        b.run()
        cen = b.heavy_census()
        want = expected_census(w["sh"], var)
        print(f"\n{label(var)}: census {cen}")
        assert cen == want, (cen, want)
        assert cen["chain_short"] >= 30 and cen["chain_long"] >= 30 and cen["rescue"] >= 80 and (cen["dedup"] >= 90 or var.get("ARX_DEDUP_HEAVY") == 0)
        if var.get("ARX_RESCUE_LDS_CLASSES"):
            assert min(cen["rescue_170"], cen["rescue_340"], cen["rescue_680"]) >= 4, cen
        check_batch(w, b, var)
        if not var:      # the default variant: the Go half and the post passes as well, and the compiled reference where it is present
            n_pairs = len(w["lens"]) // 2
            po, flags = [0, n_pairs // 2, n_pairs], [True, True]
            names, offs, clens, alt, l_pac = w["ref"].contigs()
            orfa = rfadrv.oracle_rfa(w["ora"], w["lens"], po, flags, l_pac, offs)
            parity.check_rfa(b.rfa(po, flags), orfa)
            parity.check_post(b.post(), rfadrv.oracle_post(w["o"].h, w["ora"], w["flat"], w["lens"], po, offs, orfa))
            import refdrv
            if refdrv.available():
                r = refdrv.Ref(w["fa"])
                parity.check_final(b.fetch(), r.batch(w["flat"], w["lens"], n_threads=8))
                r.close()
    finally:
        b.free()


def test_same_batch_twice_and_in_halves_in_one_handle(wl, monkeypatch):
    """One handle: the whole batch, the whole batch again, then its two halves -- the heavy lists, their cursors and the LDS staging start clean
    every time, and the census is that of each run's own reads."""
    w = wl
    set_env(monkeypatch, {})
    n = len(w["lens"])
    half = (n // 4) * 2
    b = w["ref"].batch(w["flat"], w["lens"])
    try:
        for k, (r0, r1) in enumerate(((0, n), (0, n), (0, half), (half, n))):
            if k:
                b.reset(w["flat"][w["off"][r0]:w["off"][r1]], w["lens"][r0:r1])
            b.heavy_census(True)
            b.run()
            cen = b.heavy_census()
            assert cen == expected_census(w["sh"], {}, reads=slice(r0, r1)), (r0, r1, cen)
            check_batch(w, b, {}, r0, r1)
    finally:
        b.free()

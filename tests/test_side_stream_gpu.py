"""The side stream (HipRT::on_aux) on the GPU against the restatement, every part on and off (-m gpu).

With the side streams on, a batch's narrow launches run beside the wide launch of the same stage: the rescue replay of the heavy pairs beside
the thread-per-pair launch; after a classification pass the light reads' chaining, KChainMid (the reads above k_chain_heavy's cap of 832
occurrences, one thread each) and both k_chain_heavy launches side by side (ARX_CHAIN_SPLIT=0: KChainMid beside the heavy launches after
KChain); k_dedup_heavy beside KDedup after a pass that lists its reads; CIGAR band class 2 beside the other classes.  What can go wrong is a
launch that starts before what it reads is written, a join that comes after a host read-back or an arena rewind, or two launches writing
one slot.

Workload: the 1,000-read recipe of test_launch_paths_gpu.py (nasty_reads seed 21, two barcodes of 250 pairs) on test_seed_lists_gpu.py's 340 kb
genome with its planted families of 500, 501 and 1,100 exact copies, with the heavy kernels' thresholds lowered as there, and three more
pairs built from the planted units: reads of three units (3 x 500 occurrences after occ_fill's cap: above 832, KChainMid's) and reads of one
unit and unique sequence (about 500: k_chain_heavy's long launch).  That every list the forks are about is non-empty is asserted from the
restatement before the device is looked at.

Every variant must give the restatement's final regions, alignment records, CIGARs (parity.check_final) and placed candidates
(parity.check_rfa), and all variants the same bytes; so must the same batch run twice in one handle (events and arena reused) and two handles
driven by two host threads at once (four streams)."""
import os
import tempfile
import threading

import numpy as np
import pytest

import cigarcases as cc
import parity
import rfadrv
import workloads
from arachne_amd import api

pytestmark = pytest.mark.gpu

THRESHOLDS = {"ARX_CHAIN_HEAVY_MIN": 12, "ARX_DEDUP_HEAVY_MIN": 3, "ARX_RESCUE_HEAVY_MIN": 6}    # test_launch_paths_gpu's
CHAIN_LDS_SMALL, CHAIN_LDS_OCC = 256, 832                                                         # pipeline.h
PARTS = ("ARX_AUX_RESCUE", "ARX_AUX_CHAIN", "ARX_CHAIN_SPLIT", "ARX_AUX_DEDUP", "ARX_AUX_NW")      # each part's own switch, beneath ARX_AUX_STREAM


def parts(*on):
    return {"ARX_AUX_STREAM": 1, **{p: int(p in on) for p in PARTS}}


ALL_ON = parts(*PARTS)
VARIANTS = [
    ALL_ON,
    {"ARX_AUX_STREAM": 0},
    parts("ARX_AUX_RESCUE"),
    parts("ARX_AUX_CHAIN"),                                                                       # KChainMid beside the heavy launches, after KChain
    parts("ARX_AUX_CHAIN", "ARX_CHAIN_SPLIT"),                                                    # classification pass, then three side by side
    parts("ARX_CHAIN_SPLIT"),                                                                     # (beneath a part that is off: nothing forks)
    parts("ARX_AUX_DEDUP"),
    parts("ARX_AUX_NW"),
    {k: 0 for k in PARTS},                                                                        # the master switch at its default, no part
    {},                                                                                           # the defaults, whatever they are
]
KNOBS = sorted({k for v in VARIANTS for k in v} | set(THRESHOLDS))


def label(var):
    if all(p in var for p in PARTS):               # the parts that are on, by name
        on = "+".join(p[4:] for p in PARTS if var[p]) or "no part"
        return on if "ARX_AUX_STREAM" in var else on + " (master unset)"
    return ",".join(f"{k[4:]}={v}" for k, v in var.items()) or "default"


def set_env(monkeypatch, var):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**THRESHOLDS, **var}.items():
        monkeypatch.setenv(k, str(v))


def occurrences(o, seq):
    """Seed occurrences of one read as mem_chain takes them from its intervals (bwamem.c:271-276): at most max_occ = 500 per interval, evenly
    stepped; an interval is (k, l, size, begin << 32 | end)."""
    total = 0
    for s in o.collect_intv(seq)[:, 2].astype(np.int64):
        step = max(int(s) // 500, 1)
        total += min(-(-int(s) // step), 500)
    return total


def planted_reads(g, units, rng):
    """Three pairs of 150-base reads from the planted units.  A copy in the genome is preceded by u[-1] + 1 and followed by u[0] + 1 (mod 4); a unit
    here is preceded by u[-1] + 2 and followed by u[0] + 2, so its SMEM is the unit itself with all of the family's rows."""
    def spaced(parts):
        out = []
        for k, u in enumerate(parts):
            if k:
                sp = rng.integers(0, 4, size=15, dtype=np.uint8)
                sp[0], sp[-1] = (parts[k - 1][0] + 2) % 4, (u[-1] + 2) % 4
                out.append(sp)
            out.append(u)
        r = np.concatenate(out)
        assert len(r) == 150
        return r

    def unit_and_unique(u):
        c1 = g.seqs[1]
        p = int(rng.integers(1000, len(c1) - 300))
        t = c1[p:p + 110].copy()
        t[0] = (u[0] + 2) % 4
        return np.concatenate([u, t])
    u500, u501, u1100 = units
    fwd = [spaced([u500, u501, u1100]), unit_and_unique(u500), spaced([u1100, u1100, u501])]
    rev = [spaced([u1100, u500, u500]), unit_and_unique(u501), unit_and_unique(u1100)]
    reads = []
    for a, b in zip(fwd, rev):
        reads += [a, workloads._rc(b)]
    return np.array(reads, dtype=np.uint8)


def band_classes(o, seqs, ora):
    """Queued regions per CIGAR band class, from the restatement's regions and its shape rows of mem_reg2aln on the gapped ones."""
    rows = ora["regs"]
    read_of = np.repeat(np.arange(len(ora["reg_off"]) - 1), np.diff(ora["reg_off"]))
    l1, l2 = rows[:, cc.COL["qe"]] - rows[:, cc.COL["qb"]], rows[:, cc.COL["re"]] - rows[:, cc.COL["rb"]]
    gapped = np.flatnonzero(~((l1 == l2) & (l1 - rows[:, cc.COL["truesc"]] < 12)))
    flat = dict(rows=rows[gapped], read_of=read_of[gapped], reads=seqs)
    return cc.census_from_shapes(flat, cc.expected(o, flat)["shapes"])["per_class"]


@pytest.fixture(scope="module")
def wl(built):
    import oradrv
    import test_seed_lists_gpu as seed_lists
    g, flat, lens, tags = seed_lists._workload()
    off = np.concatenate([[0], np.cumsum(lens)])
    unit_reads = [flat[off[i]:off[i + 1]] for i in np.flatnonzero(np.array(tags) == "unit")]
    units = unit_reads[0::3]                       # per family: the unit, its reverse complement, the unit between random flanks
    assert [len(u) for u in units] == [seed_lists.UNIT] * 3
    rs = workloads.nasty_reads(21, g, n_barcodes=2, pairs_per_barcode=250)
    assert rs.seqs.shape == (1000, 150)
    extra = planted_reads(g, units, np.random.default_rng(77))
    seqs = np.vstack([rs.seqs, extra])
    lens = np.full(len(seqs), 150, dtype=np.int32)
    po = rs.pair_offsets().copy()
    po[-1] += len(extra) // 2                      # the planted pairs ride in the last barcode
    flags = [rfadrv.worth_running_rfa(rs.barcodes[i], int(po[i + 1] - po[i])) for i in range(len(po) - 1)]
    assert flags == [True, True]
    d = tempfile.mkdtemp(prefix="arx_side_stream_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    g.write_alt(fa + ".alt")
    api.index_build(fa, fa)
    o = oradrv.Oracle(fa)
    # what the forks are about, from the restatement alone
    occ = np.array([occurrences(o, s) for s in seqs])
    core = np.array([len(o.align1(s)) for s in seqs])
    ora = o.batch(seqs, lens, n_threads=8)
    classes = band_classes(o, seqs, ora)
    have = dict(above_cap=int((occ > CHAIN_LDS_OCC).sum()), chain_long=int(((occ > CHAIN_LDS_SMALL) & (occ <= CHAIN_LDS_OCC)).sum()),
                chain_short=int(((occ >= 12) & (occ <= CHAIN_LDS_SMALL)).sum()), dedup=int(((core >= 3) & (core <= 256)).sum()),
                rescue=int((core[0::2] + core[1::2] >= 6).sum()), band_classes=classes)
    print(f"\nside-stream workload: {have}")
    assert have["above_cap"] >= 1 and have["chain_long"] >= 1 and have["chain_short"] >= 1 and have["dedup"] >= 1 and have["rescue"] >= 1, have
    assert sum(1 for c in classes if c > 0) >= 2, classes
    ref = api.load_reference(fa, 0)
    names, offs, clens, alt, l_pac = ref.contigs()
    want_rfa = rfadrv.oracle_rfa(ora, lens, po, flags, l_pac, offs)
    yield dict(ref=ref, seqs=seqs, lens=lens, po=po, flags=flags, ora=ora, want_rfa=want_rfa, have=have)
    ref.close()
    o.close()


def as_bytes(dev, cands):
    out = []
    for d in (dev, cands):
        for k in sorted(d):
            if isinstance(d[k], np.ndarray):
                out.append((k, d[k].tobytes()))
    return out


def finish(w, b):
    """fetch, place, compare with the restatement -> the bytes of everything fetched"""
    dev = b.fetch()
    cands = b.rfa(w["po"], w["flags"])
    parity.check_final(dev, w["ora"])
    parity.check_rfa(cands, w["want_rfa"])
    assert int((cands["cands"]["active"] == 1).sum()) == len(w["lens"])      # one placement per read
    return as_bytes(dev, cands)


first = {}      # the first variant's bytes: every later one equals them


def same_as_first(got, what):
    want = first.setdefault("bytes", got)
    differ = [k for (k, a), (_, b) in zip(got, want) if a != b]
    assert len(got) == len(want) and not differ, (what, differ)


@pytest.mark.parametrize("var", VARIANTS, ids=[label(v) for v in VARIANTS])
def test_variant_equals_restatement_and_the_others(wl, monkeypatch, var):
    set_env(monkeypatch, var)
    b = wl["ref"].batch(wl["seqs"], wl["lens"])
    try:
        b.heavy_census(True)
        b.run()
        cen = b.heavy_census()
        print(f"\n  {label(var)}: heavy census {cen}")
        assert cen["chain_short"] > 0 and cen["chain_long"] > 0 and cen["dedup"] > 0 and cen["rescue"] > 0, cen
        assert (cen["chain_short"], cen["chain_long"]) == (wl["have"]["chain_short"], wl["have"]["chain_long"]), (cen, wl["have"])
        if var == ALL_ON:                       # every part on: the chaining ran split, and its classification is the restatement's
            who, heavy, mid, asked, cap = b.debug_chain_class()
            assert len(heavy) == cen["chain_short"] + cen["chain_long"] and (who[heavy] == 1).all() and int((who == 1).sum()) == len(heavy)
            assert asked == len(mid) == wl["have"]["above_cap"] and (who[mid] == 2).all() and int((who == 2).sum()) == len(mid)
            assert cap == len(wl["lens"]) // 4 + 64
        same_as_first(finish(wl, b), label(var))
    finally:
        b.free()


def test_same_batch_twice_in_one_handle(wl, monkeypatch):
    """events, the side stream and the arena are those of the first run"""
    set_env(monkeypatch, ALL_ON)
    b = wl["ref"].batch(wl["seqs"], wl["lens"])
    try:
        for k in range(2):
            if k:
                b.reset(wl["seqs"], wl["lens"])
            b.run()
            same_as_first(finish(wl, b), "run %d of one handle" % (k + 1))
    finally:
        b.free()


def test_two_handles_on_two_host_threads(wl, monkeypatch):
    """two main and two side streams at once"""
    set_env(monkeypatch, ALL_ON)
    got, errors = [None, None], []

    def work(i):
        try:
            b = wl["ref"].batch(wl["seqs"], wl["lens"])
            try:
                b.run()
                got[i] = finish(wl, b)
            finally:
                b.free()
        except BaseException as e:     # (an assertion in a thread would otherwise pass unseen)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        same_as_first(got[i], "handle %d of two" % i)

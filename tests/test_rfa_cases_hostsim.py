"""The planted placement cases (tests/rfacases.py) on the CPU: first the cases themselves are held to what they claim, from the restatement's output
alone (oracle/arx_oracle_rfa.c) -- candidate and surviving-molecule counts per barcode, reads that change their active candidate between a run
without and a run with RFA, the index of the sink they end in, both arg-max ties, sum_move and best_in_mol values that differ from their
defaults.  Then the host double's arx_selftest_rfa, which compiles the product's pipeline_rfa.h and dev_rfa.h, runs the same batch in three
lane orders and is compared with the restatement field by field (parity.check_rfa).  tests/test_rfa_cases_gpu.py runs the batch on the GPU."""
import os
import subprocess
import time

import numpy as np
import pytest

import rfacases

SIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "libarx_hostsim.so")
ACTIVE, MAPQ, MOL, FILTERED, SUM_MOVE, BEST_IN_MOL = 12, 14, 15, 17, 18, 19


@pytest.fixture(scope="module")
def case(built):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    c = rfacases.build()
    t0 = time.time()
    c["ora"] = rfacases.oracle(c)
    c["ora_seconds"] = time.time() - t0
    c["ora_off"] = rfacases.oracle(c, np.zeros(len(c["barcodes"]), dtype=np.uint8))
    print(f"\n[rfa cases] {len(c['barcodes'])} barcodes, {c['n_reads']} reads, {len(c['ora']['cands'])} candidates; restatement {c['ora_seconds']:.1f} s")
    return c


def _slices(case):
    po, off = case["bc_pair_off"], case["ora"]["cand_off"]
    for i, b in enumerate(case["barcodes"]):
        yield i, b, int(2 * po[i]), int(off[2 * po[i]]), int(off[2 * po[i + 1]])


def _active_listing(ora, read):
    lo, hi = int(ora["cand_off"][read]), int(ora["cand_off"][read + 1])
    act = np.flatnonzero(ora["cands"][lo:hi, ACTIVE] == 1)
    assert len(act) == 1, read
    return int(act[0]), lo


def test_restatement_work_is_bounded(case):
    """What bounds the restatement's time is the size of the largest barcodes, so that is what is held (its time is printed by the fixture: about
    2 s, mostly the 2049-molecule barcode; the barcode must stay above 1024 surviving molecules)."""
    sizes = {b.name: (b.n_c, b.n_mol) for b in case["barcodes"]}
    assert sizes["molecules=2049"] == (4143, 2049) and max(n for n, _ in sizes.values()) == 6003 and len(case["ora"]["cands"]) < 45000


def test_planted_counts(case):
    rows = case["ora"]["cands"]
    names = [b.name for b in case["barcodes"]]
    for n in rfacases.EDGE_N_C:
        assert f"n_c={n}" in names
    for n in rfacases.MOLECULES:
        assert f"molecules={n}" in names
    mid = names.index("no RFA")
    assert 0 < mid < len(names) - 1 and not case["barcodes"][mid].do_rfa and case["do_rfa"].sum() == len(names) - 1
    for i, b, r0, lo, hi in _slices(case):
        assert hi - lo == b.n_c, (b.name, hi - lo, b.n_c)
        n_mol = int(rows[lo:hi, MOL].max()) + 1
        assert n_mol == (b.n_mol if b.do_rfa else 0), (b.name, n_mol, b.n_mol)
        if (b.n_c >= 255 and b.name.startswith("n_c=")) or b.n_c >= 1000:   # large: the n_c edge barcodes from 255 on and whatever holds 1,000 candidates
            assert (rows[lo:hi, FILTERED] == 0).any(), b.name          # unfiltered candidates inside every large barcode
    assert sum(rfacases.small_class_rule(case)) >= 3
    assert sum(1 for b in case["barcodes"] if b.n_c > 4096) >= 2        # P = 8192: the sort in HBM


def test_reads_move_and_ties_resolve(case):
    on, off = case["ora"], case["ora_off"]
    rows = on["cands"]
    n_moved, ties = 0, 0
    for i, b, r0, lo, hi in _slices(case):
        if not b.do_rfa:
            continue
        for pair, expect, min_sink in b.claims["movers"]:
            for read in (r0 + 2 * pair, r0 + 2 * pair + 1):
                a0, _ = _active_listing(off, read)
                a1, base = _active_listing(on, read)
                assert (a0, a1) == (0, expect), (b.name, pair, a0, a1, expect)
                assert rows[base + a1, MOL] >= min_sink, (b.name, pair, rows[base + a1, MOL], min_sink)
                n_moved += 1
        for pair, expect, what in b.claims["ties"]:
            read = r0 + 2 * pair
            a1, base = _active_listing(on, read)
            mols = rows[base:int(on["cand_off"][read + 1]), MOL]
            other = [int(m) for k, m in enumerate(mols) if k not in (0, expect)]
            assert a1 == expect and other, (b.name, what)
            if "smaller wins" in what:
                assert all(mols[expect] < m for m in other), (b.name, what, mols)
                assert ((int(mols[expect]) % 1024) >> 6) != ((other[0] % 1024) >> 6), (b.name, what, mols)   # argmax meets sink T in lane T % 1024: different waves
            else:
                assert all(mols[expect] > m for m in other), (b.name, what, mols)
            ties += 1
    assert n_moved > 400 and ties == 3
    named = {b.name: b for b in case["barcodes"]}
    assert max(m for _, _, m in named["molecules=65"].claims["movers"]) >= 64
    for n in ("molecules=1025", "molecules=2049"):
        assert max(m for _, _, m in named[n].claims["movers"]) >= 1024


def test_molecules_split_above_50000(case):
    """Neighbours exactly 50,000 apart share a molecule, exactly 50,001 apart do not (aligner.go inferMolecules: > 50000); all three pairs stay active."""
    on = case["ora"]
    rows, n = on["cands"], 0
    for i, b, r0, lo, hi in _slices(case):
        for pa, pb, pc in b.claims.get("neighbours", []):
            c = [rows[int(on["cand_off"][r0 + 2 * p]):int(on["cand_off"][r0 + 2 * p + 2])] for p in (pa, pb, pc)]
            assert all(len(x) == 2 and (x[:, ACTIVE] == 1).all() for x in c)
            assert c[1][0, 2] - c[0][1, 2] == 50_000 and c[2][0, 2] - c[1][1, 2] == 50_001     # sorted neighbours: A's reverse read, B's forward read, ...
            mols = [set(int(m) for m in x[:, MOL]) for x in c]
            assert all(len(m) == 1 and min(m) >= 0 for m in mols) and mols[0] == mols[1] and mols[2] == {min(mols[1]) + 1}, mols
            n += 1
    assert n == 2


def test_fields_leave_their_defaults(case):
    rows = case["ora"]["cands"]
    sm = rows[:, SUM_MOVE].copy().view(np.float64)
    assert (sm != 1.0).any() and (sm >= 1.0).all()
    assert ((rows[:, BEST_IN_MOL] == 1) & (rows[:, ACTIVE] == 0)).any()
    assert set(np.unique(rows[:, BEST_IN_MOL])) == {0, 1}
    # a moved read whose former placement is molecule 0 of its barcode: its sum runs over sink 0
    hit = 0
    for i, b, r0, lo, hi in _slices(case):
        for pair, expect, _ in b.claims["movers"] if b.do_rfa else []:
            a1, base = _active_listing(case["ora"], r0 + 2 * pair)
            if rows[base, MOL] == 0 and sm[base + a1] > 1.0:
                hit += 1
    assert hit >= 10
    # the centromere of contig 1: unique pairs inside it get MAPQ 0, the same pairs elsewhere 60
    act = rows[rows[:, ACTIVE] == 1]
    inside = (act[:, 5] == 1) & (act[:, 2] > rfacases.CENTROMERES[0][1]) & (act[:, 2] <= rfacases.CENTROMERES[1][1])
    assert inside.sum() >= 20 and (act[inside, MAPQ] == 0).all() and (act[~inside, MAPQ] == 60).sum() > 1000
    # candidates of different reads at equal positions
    for i, b, r0, lo, hi in _slices(case):
        if b.name == "n_c=4097":
            f = rows[lo:hi][rows[lo:hi, FILTERED] == 1]
            key = f[:, 5] * (1 << 40) + f[:, 2]
            u, cnt = np.unique(key, return_counts=True)
            assert (cnt >= 2).sum() > 100


@pytest.mark.parametrize("lane_order", [0, 1, 2])
def test_host_double_matches_restatement(case, lane_order, monkeypatch):
    monkeypatch.setenv("ARX_SIM_PFOR", str(lane_order))
    t0 = time.time()
    dev = rfacases.run_device(case, SIM)
    print(f"\n[rfa cases] host double, lane order {lane_order}: {time.time() - t0:.1f} s, n_host_mapq {dev['n_host_mapq']}")
    rfacases.check_device(case, dev, np.zeros(len(case["barcodes"]), dtype=np.uint8))


def test_host_double_class_rule_and_guard(case):
    """The class bytes follow the rule where rfa_small is on (the double launches every barcode the same way: only the bytes are looked at); with
    the guard at 0.6 the host re-evaluates and patches every read (RfaStage::run: a guard of 0.5 and more leaves no value outside the band)."""
    dev = rfacases.run_device(case, SIM, rfa_small=True, mapq_guard=0.6)
    print(f"\n[rfa cases] host double, guard 0.6: n_host_mapq {dev['n_host_mapq']} of {case['n_reads']} reads")
    rfacases.check_device(case, dev, rfacases.small_class_rule(case))
    assert dev["n_host_mapq"] == case["n_reads"]

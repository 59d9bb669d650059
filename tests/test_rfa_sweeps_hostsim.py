"""The placement kernel sweeps only the sources that can move a read (dev_rfa.h: a molecule is flagged where a read with spots in two or more
molecules has one of them in it; ARX_RFA_SKIP_SWEEPS=0 sweeps every source), on the CPU.

First the batch of tests/rfasweeps.py is held to the shapes it claims, from the restatement's output alone (oracle/arx_oracle_rfa.c).  Then the
host double's arx_selftest_rfa, which compiles the product's pipeline_rfa.h and dev_rfa.h, runs it with the switch on and off in three lane
orders: every candidate field, sum_move bit for bit, best_in_mol and the molecule count per barcode equal the restatement's, the two forms
are byte-identical, and the sweeps a barcode ran (the `pad` word of its output record) are what the rule says.  Last the benchmark's read
recipe through the whole double: the share of barcodes with any flagged molecule.

A barcode with RFA and no surviving molecule (cnt = 0) cannot be built: tagBestAlignments makes one candidate of every read active, a read
without hits included (its placeholder lies at position -1 of contig ""), and a molecule that holds an active alignment survives.  The
barcode without RFA is the one that reports no molecule."""
import os
import subprocess
import tempfile
import time

import numpy as np
import pytest

import parity
import rfacases
import rfadrv
import rfasweeps
from rfasweeps import ACTIVE, MOL, SWITCH

SIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "libarx_hostsim.so")


@pytest.fixture(scope="module")
def case(built):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    c = rfasweeps.build()
    c["ora"] = rfacases.oracle(c)
    c["ora_off"] = rfacases.oracle(c, np.zeros(len(c["barcodes"]), dtype=np.uint8))
    c["census"] = rfasweeps.census(c["ora"], c["bc_pair_off"])
    return c


def _reads(case, role):
    i = case["shape"][role]
    return i, 2 * int(case["bc_pair_off"][i]), 2 * int(case["bc_pair_off"][i + 1])


def test_shapes_from_the_restatement(case):
    cen, sh = case["census"], case["shape"]
    for cnt in (1, 2, 4, 9):                                       # no read with two spots
        i, r0, r1 = _reads(case, f"plain{cnt}")
        assert cen[i] == (cnt, set(), 0), (cnt, cen[i])
        assert rfasweeps.moved_reads(case["ora"], case["ora_off"], r0, r1) == 0
    i = sh["plain4"]                                               # ... though reads with several placements are among them
    lo, hi = (int(case["ora"]["cand_off"][2 * case["bc_pair_off"][k]]) for k in (i, i + 1))
    assert hi - lo > 2 * (case["bc_pair_off"][i + 1] - case["bc_pair_off"][i]) and (case["ora"]["cands"][lo:hi, MOL] < 0).any()
    for role in ("first", "last", "accepted"):                     # exactly one flagged pair of molecules among unflagged ones, two reads
        i, r0, r1 = _reads(case, role)
        lone, dense = sh[role + "_mols"]
        cnt, flagged, n2 = cen[i]
        assert flagged == {lone, dense} and n2 == 2 and cnt >= 7, (role, cen[i])
        assert rfasweeps.moved_reads(case["ora"], case["ora_off"], r0, r1) == 2, role   # the lone source's move is accepted
    assert sh["first_mols"][0] == 0                                # the source that moves is the first of the round robin ...
    assert sh["last_mols"][0] == cen[sh["last"]][0] - 1            # ... and the last
    lone, dense = sh["accepted_mols"]                              # after the accepted move the walk passes unflagged sources on both sides
    assert 0 < lone < dense < cen[sh["accepted"]][0] - 1
    i = sh["m65"]
    assert cen[i][0] == 65 and cen[i][1] == {63, 64}               # a flagged molecule beyond a 64-bit mask
    i = sh["no_rfa"]
    assert not case["barcodes"][i].do_rfa and cen[i][0] == 0 and 0 < i < len(case["barcodes"]) - 1


def test_ladder_reaches_the_bound(case):
    """Nine rungs could be taken, one per round of the round robin; Optimize's 8 * cnt iterations are eight rounds.  The restatement takes the
    upper eight and leaves the lowest pair where it was although its molecule holds six active alignments by then -- the walk was cut short, not
    idle.  (The sweep count below says the same of the kernel: 8 * cnt sweeps in R5.)"""
    i, r0, r1 = _reads(case, "ladder")
    on, rungs = case["ora"], case["shape"]["ladder_rungs"]
    cnt, flagged, _ = case["census"][i]
    assert cnt == 11 and flagged == set(range(11)) and len(rungs) == 9
    where = []
    for p in rungs:
        lo, hi = int(on["cand_off"][r0 + 2 * p]), int(on["cand_off"][r0 + 2 * p + 1])
        assert hi - lo == 2
        where.append(int(np.flatnonzero(on["cands"][lo:hi, ACTIVE] == 1)[0]))
    assert where == [0] + [1] * 8, where
    assert rfasweeps.moved_reads(on, case["ora_off"], r0, r1) == 16
    lo, hi = int(on["cand_off"][r0]), int(on["cand_off"][r1])
    rows = on["cands"][lo:hi]
    assert ((rows[:, ACTIVE] == 1) & (rows[:, MOL] == 2)).sum() == 6      # X_1: the next to give, had the walk gone on


@pytest.fixture(scope="module")
def runs(case):
    """(lane order, switch) -> result of the double; the environment is put back"""
    keep = {k: os.environ.get(k) for k in (SWITCH, "ARX_SIM_PFOR")}
    out = {}
    try:
        for order in (0, 1, 2):
            for sw in (1, 0):
                os.environ["ARX_SIM_PFOR"], os.environ[SWITCH] = str(order), str(sw)
                t0 = time.time()
                out[order, sw] = rfacases.run_device(case, SIM)
                print(f"\n[rfa sweeps] host double, lane order {order}, {SWITCH}={sw}: {time.time() - t0:.2f} s, sweeps per barcode {out[order, sw]['barcodes']['pad'].tolist()}")
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("sw", [1, 0])
def test_host_double_matches_restatement(case, runs, order, sw):
    rfacases.check_device(case, runs[order, sw], np.zeros(len(case["barcodes"]), dtype=np.uint8))


def test_both_forms_are_byte_identical(runs):
    for k in runs:
        rfasweeps.same_results(runs[0, 1], runs[k])


def test_sweep_counts(case, runs):
    for order in (0, 1, 2):
        rfasweeps.check_sweep_counts(case, runs[order, 1], runs[order, 0])
        assert (runs[order, 1]["barcodes"]["pad"] == runs[0, 1]["barcodes"]["pad"]).all()


def test_bench_like_census(built):
    """130 barcodes x 77 pairs by the benchmark's read recipe (tests/extclosed.py) through the whole double with the placement stage: equal to
    the restatement, and how many barcodes the walk still has to sweep at all."""
    import oradrv
    from arachne_amd import api
    from extclosed import bench_like_inputs
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    g, rs = bench_like_inputs()
    fa = os.path.join(tempfile.mkdtemp(prefix="arx_rfasw_"), "g.fa")
    g.write_fasta(fa)
    api.index_build(fa, fa, lib_path=SIM)
    ref = api.Reference(fa, lib_path=SIM)
    o = oradrv.Oracle(fa)
    try:
        ora = o.batch(rs.seqs, rs.lens, n_threads=8)
        po = rs.pair_offsets()
        flags = np.ones(len(po) - 1, dtype=np.uint8)
        names, offs, clens, alt, l_pac = ref.contigs()
        b = ref.batch(rs.seqs, rs.lens).run()
        cands = b.rfa(po, flags)
        b.free()
        orfa = rfadrv.oracle_rfa(ora, rs.lens, po, flags, l_pac, offs)
        parity.check_rfa(cands, orfa)
    finally:
        ref.close()
        o.close()
    cen = rfasweeps.census(orfa, po)
    n_bc = len(cen)
    cnts = np.array([c[0] for c in cen])
    with_flag = sum(1 for c in cen if c[1])
    mols, flagged = int(cnts.sum()), sum(len(c[1]) for c in cen)
    print(f"\n[rfa sweeps] bench-like census: {n_bc} barcodes, cnt mean {cnts.mean():.2f} max {cnts.max()}; barcodes with a flagged molecule {with_flag} "
          f"({100.0 * with_flag / n_bc:.1f} %); flagged molecules {flagged} of {mols} ({100.0 * flagged / mols:.1f} %)")
    assert n_bc == 130 and mols > 0

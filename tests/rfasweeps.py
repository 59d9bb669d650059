"""What the sweep-skip tests share (test_rfa_sweeps_hostsim.py, test_rfa_sweeps_gpu.py): one batch of barcodes built with tests/rfacases.py's
blocks around the rule "only a source that holds a read with spots in two or more molecules is swept" (dev_rfa.h), and the quantities of that
rule computed from the restatement's output alone.

A read's spots are its candidates with best_in_mol = 1 in a surviving molecule (molecule_id >= 0); a molecule is flagged where a read with two
or more spots has one of them in it.  The fastScore sweeps a barcode ran come back in the `pad` word of its output record (dev_rfa.h
RfaBarcodeOut), which no comparison reads."""
import numpy as np

import rfacases
from rfacases import Barcode, fwd, rev

READ, ACTIVE, MOL, SUM_MOVE, BEST_IN_MOL = 1, 12, 15, 18, 19
SWITCH = "ARX_RFA_SKIP_SWEEPS"


def plain(cnt):
    """cnt surviving molecules and no read with two spots: isolated pairs; from four molecules on one of them dense, one pair with an unfiltered extra
    placement and one with three equal placements of which two lie in regions that hold nothing active (their molecules disappear, the spots with them)."""
    b = Barcode(f"plain cnt={cnt}")
    if cnt < 4:
        for _ in range(cnt):
            b.iso()
        return b
    b.iso()
    s = b.dense(0, 6, span=6000)
    b.pair([fwd(s + 4300), fwd(s + 4350, score=100)], [rev(s + 4500)])
    b.iso()
    far = [b.region(0, 200, live=(i == 0)) for i in range(3)]
    b.pair([fwd(x) for x in far], [rev(x + 200) for x in far])
    for _ in range(cnt - 4):
        b.iso()
    assert b.n_mol == cnt
    return b


def one_flagged_pair(name, before, between, after, dense_pairs=6):
    """`before` isolated pairs, a lone region, `between` isolated pairs, a dense molecule, `after` isolated pairs; one pair lies in the lone region
    (listed first: tagBestAlignments keeps it there) and inside the dense molecule.  Its two reads are the only ones with two spots, the lone and
    the dense molecule the only flagged ones; fastScore(lone -> dense) > 0 (the source empties), so the walk moves both reads when it sweeps the
    lone molecule.  -> (barcode, index of the lone molecule, index of the dense one)"""
    b = Barcode(name)
    for _ in range(before):
        b.iso()
    lone = b.region(0, 200)
    for _ in range(between):
        b.iso()
    d = b.dense(0, dense_pairs, span=6000)
    for _ in range(after):
        b.iso()
    p = b.pair([fwd(lone), fwd(d + 250)], [rev(lone + 200), rev(d + 450)])
    b.claims["movers"].append((p, 1, before + between + 1))
    return b, before, before + between + 1


def dense_then_lone(name, before, after):
    """As one_flagged_pair with the dense molecule in front of the lone one: the lone source comes last of the two in round-robin order."""
    b = Barcode(name)
    for _ in range(before):
        b.iso()
    d = b.dense(0, 6, span=6000)
    lone = b.region(0, 200)
    for _ in range(after):
        b.iso()
    p = b.pair([fwd(lone), fwd(d + 250)], [rev(lone + 200), rev(d + 450)])
    b.claims["movers"].append((p, 1, before))
    return b, before + 1, before


def ladder(n):
    """A walk that is still moving reads when it reaches the 8 * cnt bound.  Molecule 0 is a large dense one, D; molecules 1 .. n are X_0 .. X_{n-1}.
    Every X_i holds two pairs, A_i and B_i (four active alignments: not an active molecule, which takes more than four); the top one, X_{n-1},
    a third, W (six: active).  B_i also lies in X_{i-1}, listed second.  i pairs of D also lie in X_i, listed second ("visitors": they add
    2 * i spots to X_i and never move -- D gains nothing by giving them).  fastScore of moving B_i down: a source that falls from six to four
    active alignments stops being active, + its spots (6 + 2 * i); a sink that rises from four to six becomes active, - its spots
    (6 + 2 * (i - 1)); the reads' own terms are 0.  So a molecule of six gives B_i to the one below for + 2 and a molecule of four gives nothing
    (- spots of the sink).  Sources are visited in ascending order and the ladder descends: X_{n-1} gives in the first round, X_{n-2}, six by
    then, in the second, one rung per round.  Optimize allows 8 rounds (8 * cnt iterations): of the n - 1 rungs the first eight are taken.
    -> (barcode, pairs B_1 .. B_{n-1})"""
    b = Barcode(f"ladder {n}")
    n_vis = n * (n - 1) // 2
    d = b.region(0, (n_vis + 6) * 700 + 200)
    xs = [b.region(0, 6000) for _ in range(n)]
    for j in range(6):
        b.pair([fwd(d + 700 * j)], [rev(d + 700 * j + 200)])
    j = 6
    for i, s in enumerate(xs):
        for k in range(i):
            b.pair([fwd(d + 700 * j), fwd(s + 3000 + 30 * k)], [rev(d + 700 * j + 200), rev(s + 3200 + 30 * k)])
            j += 1
    rungs = []
    for i, s in enumerate(xs):
        b.pair([fwd(s)], [rev(s + 200)])
        if i == 0:
            b.pair([fwd(s + 700)], [rev(s + 900)])
        else:
            rungs.append(b.pair([fwd(s + 700), fwd(xs[i - 1] + 1400)], [rev(s + 900), rev(xs[i - 1] + 1600)]))
    b.pair([fwd(xs[-1] + 2100)], [rev(xs[-1] + 2300)])
    assert b.n_mol == n + 1
    return b, rungs


def build():
    """-> the batch (as rfacases.build) with case["shape"]: barcode index by role."""
    bcs, shape = [], {}

    def add(role, b):
        shape[role] = len(bcs)
        bcs.append(b)

    for cnt in (1, 2, 4):
        add(f"plain{cnt}", plain(cnt))
    b, lone, dense = one_flagged_pair("flagged source first", 0, 0, 5)
    add("first", b); shape["first_mols"] = (lone, dense)
    add("no_rfa", Barcode("no RFA", do_rfa=False).fill_to(100))
    b, lone, dense = dense_then_lone("flagged source last", 5, 0)
    add("last", b); shape["last_mols"] = (lone, dense)
    b, lone, dense = one_flagged_pair("accepted move in the middle", 3, 0, 3)
    add("accepted", b); shape["accepted_mols"] = (lone, dense)
    b, rungs = ladder(10)
    add("ladder", b); shape["ladder_rungs"] = rungs
    add("m65", rfacases.molecules_barcode(65))
    add("plain9", plain(9))
    reads, po = [], [0]
    for b in bcs:
        reads += b.reads
        po.append(len(reads) // 2)
    return dict(barcodes=bcs, shape=shape, rows=rfacases.rows(reads, rfacases.L_PAC, rfacases.ANN_OFF), lens=np.full(len(reads), rfacases.READ_LEN, dtype=np.int32),
                bc_pair_off=np.array(po, dtype=np.int64), do_rfa=np.array([b.do_rfa for b in bcs], dtype=np.uint8), n_reads=len(reads))


def spots_of(rows):
    """rows: the restatement's candidate rows of one barcode -> (cnt, spots per read {read: [molecules]}, the set of flagged molecules)"""
    cnt = int(rows[:, MOL].max()) + 1 if len(rows) else 0
    per_read = {}
    for r in rows[(rows[:, BEST_IN_MOL] == 1) & (rows[:, MOL] >= 0)]:
        per_read.setdefault(int(r[READ]), []).append(int(r[MOL]))
    flagged = set()
    for mols in per_read.values():
        assert len(mols) == len(set(mols))      # one spot per (read, molecule)
        if len(mols) >= 2:
            flagged |= set(mols)
    return cnt, per_read, flagged


def census(ora, bc_pair_off):
    """Per barcode of a restatement result: (cnt, flagged molecules, reads with two or more spots)."""
    out = []
    off = ora["cand_off"]
    for i in range(len(bc_pair_off) - 1):
        lo, hi = int(off[2 * bc_pair_off[i]]), int(off[2 * bc_pair_off[i + 1]])
        cnt, per_read, flagged = spots_of(ora["cands"][lo:hi])
        out.append((cnt, flagged, sum(1 for m in per_read.values() if len(m) >= 2)))
    return out


def moved_reads(on, off, r0, r1):
    """reads of [r0, r1) whose active candidate differs between the restatement with and without RFA"""
    n = 0
    for read in range(r0, r1):
        lo, hi = int(on["cand_off"][read]), int(on["cand_off"][read + 1])
        n += int((on["cands"][lo:hi, ACTIVE] != off["cands"][lo:hi, ACTIVE]).any())
    return n


def same_results(a, b):
    """two api.selftest_rfa results: every byte that means something"""
    for k in ("cand_off", "cands", "cls"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("dna_len", "n_mol"):
        assert a["barcodes"][k].tobytes() == b["barcodes"][k].tobytes(), k
    assert a["n_host_mapq"] == b["n_host_mapq"]


def check_sweep_counts(case, on, off):
    """on / off: results with the switch on and off.  Without the flags every source that holds an active alignment is swept once per iteration of
    R5 and once in R6; with them only flagged ones."""
    cen, sh = case["census"], case["shape"]
    s_on, s_off = on["barcodes"]["pad"], off["barcodes"]["pad"]
    for cnt in (1, 2, 4, 9):
        i = sh[f"plain{cnt}"]
        assert s_on[i] == 0 and s_off[i] == 2 * cnt, (cnt, s_on[i], s_off[i])     # cnt idle iterations end R5, R6 visits every molecule
    for role in ("first", "last", "accepted", "m65"):
        i = sh[role]
        assert 0 < s_on[i] < s_off[i], (role, s_on[i], s_off[i])
        assert s_on[i] <= 3 * 2                                                    # two flagged sources: at most twice each in R5 (before and after the move), once in R6
    i = sh["ladder"]
    assert s_on[i] == s_off[i] == 8 * 11 + 11                                     # every molecule flagged and never empty: R5 runs into its bound
    assert s_on[sh["no_rfa"]] == 0 and s_off[sh["no_rfa"]] == 0
    assert (s_on <= s_off).all()

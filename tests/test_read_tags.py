"""arx_batch_tags: what estimateMapQualities leaves in mapq_data of every read's active alignment for AppendBam's tags -- the second
best (aligner.go:847-889), XS / AS truncated as Go's int() truncates, XM / XT, and the DM inputs of setMoleculeDifferences (:526-545).

The device result (host test double here, libarachne_amd.so under -m gpu) is compared with a plain Python restatement of the reference's
loops on the candidate records arx_batch_rfa_fetch returns: the (i, j) double loop of :863-883 with scoreAlignment (:556-581) evaluated
term by term, calculateLogMoleculePenalty (:722-755) with numpy's log10, and the per-molecule sums of setMoleculeDifferences.  Known
answers built by hand pin the corner cases: the pseudo-count XS, XT:i:1 of a barcode without RFA, a negative half-unit AS, a tie."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import workloads
from arachne_amd import api, synth

SIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "libarx_hostsim.so")
RL = 150


# ---- the restatement
def _score(a, m, penalty, lmp):
    """scoreAlignment(aln, mate, log_molecule_penalty) in the reference's order of operations; a or m may be None"""
    s = 0.0
    for x in (a, m):
        if x is None:
            continue
        s += float(x["mismatches"] * -2 + x["indels"] * -3)
        if x["soft_clipped"] > 0:
            s -= 5.0 * float(x["soft_clipped"])
            s -= float(x["soft_clipped_length"]) * 0.5
    if a is None or m is None or not _is_pair(a, m):
        s += float(penalty)
    if a is not None and not a["active_molecule"]:
        s += lmp
    return s


def _is_pair(a, b):
    if a["reversed"] == b["reversed"] or a["rid"] != b["rid"]:
        return False
    dist = int(a["pos"] - b["pos"]) if a["reversed"] else int(b["pos"] - a["pos"])
    return -35 <= dist < 750


def _log_mol_pen(cands, lo, hi, do_rfa):
    """calculateLogMoleculePenalty over the barcode's candidates [lo, hi): molecules from molecule_id, their active alignments from `active`"""
    if not do_rfa:
        return 0.0
    c = cands[lo:hi]
    mols = sorted(set(int(m) for m in c["molecule_id"] if m >= 0))
    if not mols:
        return 0.0
    dna = 1000.0
    for m in mols:
        inm = c[c["molecule_id"] == m]
        act = inm[inm["active"] == 1]
        if inm["active_molecule"].any():
            if len(act):
                dna += float(int(act["pos"].max()) - int(act["pos"].min())) + 1000.0
        else:
            for a in act:
                dna += float(a["aend"] - a["pos"]) * 2.0
    return float(np.log10(dna / 3200000000.0 * 0.05))


def restate(cands, cand_off, lens, po, flags, penalty=-4):
    out = np.zeros(len(lens), dtype=api.TAGS_DTYPE)
    for b in range(len(po) - 1):
        r0, r1 = 2 * int(po[b]), 2 * int(po[b + 1])
        lmp = _log_mol_pen(cands, cand_off[r0], cand_off[r1], flags[b])
        dm = {}
        for r in range(r0, r1):
            for i in range(cand_off[r], cand_off[r + 1]):
                if cands[i]["active"] and cands[i]["molecule_id"] >= 0:
                    n, s = dm.get(int(cands[i]["molecule_id"]), (0, 0))
                    dm[int(cands[i]["molecule_id"])] = (n + 1, s + int(cands[i]["mismatches"]))
        for r in range(r0, r1):
            own = [i for i in range(cand_off[r], cand_off[r + 1]) if cands[i]["in_filtered"]]
            mate = [j for j in range(cand_off[r ^ 1], cand_off[(r ^ 1) + 1]) if cands[j]["in_filtered"]]
            best_single = max(_score(None, cands[j], penalty, lmp) for j in mate)
            pseudo = 0.0
            pseudo -= 10.0
            pseudo -= (float(lens[r]) - 25.0) * 0.5
            pseudo += lmp
            raw, best, sb = best_single + pseudo, -1000.0, -1
            act = [i for i in own if cands[i]["active"]][-1]
            am = [j for j in mate if cands[j]["active"]][-1]
            for i in own:
                for j in mate:
                    sc = _score(cands[i], cands[j], penalty, lmp)
                    if not cands[i]["active"] and sc > best:
                        best, raw, sb = sc, _score(cands[i], cands[j], penalty, 0.0), i
            t = out[r]
            t["active"], t["second_best"], t["xs"] = act, sb, math.trunc(raw)
            t["as"] = math.trunc(_score(cands[act], cands[am], penalty, 0.0))
            if sb >= 0:
                t["xm"] = int(cands[sb]["active_molecule"])
                t["xt"] = int(cands[act]["molecule_id"] == cands[sb]["molecule_id"])
            if cands[act]["molecule_id"] >= 0:
                t["dm_n"], t["dm_sum"] = dm[int(cands[act]["molecule_id"])]
    return out


def _check(dev, exp):
    for f in api.TAGS_DTYPE.names:
        bad = np.flatnonzero(dev[f] != exp[f])
        assert len(bad) == 0, (f, bad[:5], dev[bad[:5]], exp[bad[:5]])


# ---- seeded read sets
def _workload(lib_path, kind):
    if kind == "nasty":
        g = workloads.nasty_genome(7, contig_lens=(200000, 120000, 50000), alt_contigs=1)
        rs = workloads.nasty_reads(7, g, n_barcodes=4, pairs_per_barcode=120)
    else:
        g = synth.make_genome(41, [600000, 200000])
        rs = synth.make_reads(42, g, 4, 150)
    po = rs.pair_offsets()
    flags = [api.worth_running_rfa(rs.barcodes[b], int(po[b + 1] - po[b])) for b in range(len(po) - 1)]
    if kind == "synth":
        flags[1] = False                          # one barcode takes the non-RFA branch (aligner.go:469-477)
    elif kind == "no_rfa":
        flags = [False] * len(flags)
    d = tempfile.mkdtemp(prefix="arx_tags_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    g.write_alt(fa + ".alt")
    api.index_build(fa, fa, lib_path=lib_path)
    ref = api.Reference(fa, lib_path=lib_path)
    try:
        b = ref.batch(rs.seqs, rs.lens).run()
        c = b.rfa(po, flags)
        b.post(fetch=False)
        tags = b.tags()
        b.free()
    finally:
        ref.close()
    return c, rs, po, flags, tags


def _seeded(lib_path, kind):
    c, rs, po, flags, tags = _workload(lib_path, kind)
    exp = restate(c["cands"], c["cand_off"], rs.lens, po, flags)
    _check(tags, exp)
    return tags, flags


@pytest.fixture(scope="module")
def sim(built):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    return SIM


@pytest.mark.parametrize("kind", ["synth", "nasty", "no_rfa"])
def test_tags_match_restatement_hostsim(sim, kind):
    tags, flags = _seeded(sim, kind)
    assert (tags["second_best"] >= 0).any() and (tags["second_best"] < 0).any()
    if kind != "no_rfa" and any(flags):
        assert (tags["dm_n"] > 0).any()
    else:
        assert (tags["dm_n"] == 0).all()


# ---- known answers on hand-made pairs
class Case:
    """A unique random genome with planted exact copies on contig 1: Y at 250000 twice (+30000), X at 100000 three times (+50000, +100000)."""

    def __init__(self, lib_path):
        self.g = synth.make_genome(77, [400000, 300000], repeat_families=[])
        for s in self.g.seqs:
            s[s > 3] = 0
        c1 = self.g.seqs[1]
        c1[280000:281000] = c1[250000:251000]
        c1[150000:151000] = c1[100000:101000]
        c1[200000:201000] = c1[100000:101000]
        d = tempfile.mkdtemp(prefix="arx_tags_ka_")
        self.fa = os.path.join(d, "g.fa")
        self.g.write_fasta(self.fa)
        self.g.write_alt(self.fa + ".alt")
        api.index_build(self.fa, self.fa, lib_path=lib_path)
        self.lib_path = lib_path
        self.c1 = c1

    def fwd(self, pos):
        return self.c1[pos:pos + RL].copy()

    def rev(self, pos):
        return (3 - self.c1[pos:pos + RL][::-1]).astype(np.uint8)

    def run(self, pairs, do_rfa=False):
        seqs = np.concatenate([np.concatenate(p) for p in pairs]).reshape(-1, RL)
        lens = np.full(2 * len(pairs), RL, dtype=np.int32)
        po = [0, len(pairs)]
        ref = api.Reference(self.fa, lib_path=self.lib_path)
        try:
            b = ref.batch(seqs, lens).run()
            c = b.rfa(po, [do_rfa])
            b.post(fetch=False)
            tags = b.tags()
            b.free()
        finally:
            ref.close()
        _check(tags, restate(c["cands"], c["cand_off"], lens, po, [do_rfa]))
        return c, tags


def known_answers(case):
    rng = np.random.default_rng(3)
    # 1. a unique pair: no non-active candidate, XS is the pseudo count: 0.5 * lap2(mate) + penalty - 10 - (150 - 25) / 2 + 0 = -76.5 -> -76
    c, t = case.run([(case.fwd(50000), case.rev(50250))])
    assert list(t["second_best"]) == [-1, -1] and list(t["xs"]) == [-76, -76]
    assert list(t["as"]) == [0, 0] and list(t["xm"]) == [0, 0] and list(t["xt"]) == [0, 0]
    # ... and with RFA the pseudo count carries log_molecule_penalty: one inactive molecule of two alignments, DNA length 1000 + 2 * 2 * 150
    c, t = case.run([(case.fwd(50000), case.rev(50250))], do_rfa=True)
    lmp = float(np.log10(1600.0 / 3200000000.0 * 0.05))
    assert list(t["second_best"]) == [-1, -1] and list(t["xs"]) == [math.trunc(-76.5 + lmp)] * 2 == [-84, -84]
    assert list(t["dm_n"]) == [2, 2] and list(t["dm_sum"]) == [0, 0]
    # 2. a pair inside the two copies of Y, no RFA: the other copy is the second best, both molecule ids are -1 -> XT:i:1, XS = 0
    c, t = case.run([(case.fwd(250100), case.rev(250350))])
    cand, off = c["cands"], c["cand_off"]
    assert list(off[1:] - off[:-1]) == [2, 2]
    assert list(t["xt"]) == [1, 1] and list(t["xs"]) == [0, 0] and list(t["xm"]) == [0, 0]
    for r in range(2):
        assert t["second_best"][r] >= 0 and not cand["active"][t["second_best"][r]] and cand["molecule_id"][t["second_best"][r]] == -1
    # 3. three copies of X: two non-active candidates tie at pair score 0 -- the first in candidate order wins
    c, t = case.run([(case.fwd(100100), case.rev(100350))])
    cand, off = c["cands"], c["cand_off"]
    for r in range(2):
        idle = [i for i in range(off[r], off[r + 1]) if not cand["active"][i]]
        assert len(idle) == 2 and t["second_best"][r] == idle[0] and t["xs"][r] == 0
    # 4. a soft-clipped R1 with an odd clip length: AS = int(0.5 * odd) truncates toward zero (-x.5 -> -x, not -x-1)
    tail = rng.integers(0, 4, size=RL).astype(np.uint8)
    for keep in range(112, 128):
        r1 = np.concatenate([case.fwd(60000)[:keep], tail[keep:]])
        c, t = case.run([(r1, case.rev(60250))])
        cand = c["cands"]
        a, m = int(t["active"][0]), int(t["active"][1])
        tot = int(cand["lap2"][a] + cand["lap2"][m]) + (0 if cand["is_proper"][a] else -8)
        if tot % 2:
            assert tot < 0 and t["as"][0] == -((-tot) // 2) and t["as"][1] == t["as"][0]
            return
    raise AssertionError("no odd soft-clip length found")


def test_known_answers_hostsim(sim):
    known_answers(Case(sim))


def test_tags_before_rfa_is_an_error_hostsim(sim):
    case = Case(sim)
    ref = api.Reference(case.fa, lib_path=sim)
    try:
        b = ref.batch(np.stack([case.fwd(50000), case.rev(50250)]), np.full(2, RL, dtype=np.int32)).run()
        with pytest.raises(api.ArachneError, match="before arx_batch_rfa"):
            b.tags()
        b.free()
    finally:
        ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["synth", "nasty", "no_rfa"])
def test_tags_match_restatement_gpu(built, kind):
    _seeded(api.LIB_PATH, kind)


@pytest.mark.gpu
def test_known_answers_gpu(built):
    known_answers(Case(api.LIB_PATH))

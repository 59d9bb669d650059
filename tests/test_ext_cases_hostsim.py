"""The planted extension-stage cases (tests/extcases.py) on the CPU.  First the restatement (oracle/arx_oracle.c: ora_chain2aln over the static
chain2aln) is held to what every named case says it must reach and give: the edge from its shape row and call list, the regions written down by hand.
Then the host double's arx_selftest_ext_stage, which compiles the product's pipeline.h and dev_regs.h, runs Pipeline::stage_extend on every batch in
the three item orders of its thread-per-item launches, with ARX_EXT_CLOSED set to 0 and to 1, and is compared with the restatement without a
tolerance (extcases.check_device).  Within a round the chains of a read read each other's done_round: the dependency rule (dev_regs.h) says the
answer does not depend on which of them steps first, and the three orders hold it to that.
tests/test_ext_stage_gpu.py runs the same batches on the GPU; tests/test_oracle_vs_ref.py and tests/test_oracle_golden.py hold the restatement to the
reference's mem_chain2aln on the same rows."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import extcases
import oradrv
from arachne_amd import api
from extcases import CL, SH

SIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "libarx_hostsim.so")
NAMES = ["main", "no DP", "active=63", "active=64", "active=65", "big"]


@pytest.fixture(scope="module")
def cases(built):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    c = extcases.build_all()
    fa = c["genome"].write_index(SIM)
    c["ref"] = api.Reference(fa, lib_path=SIM)
    c["drv"] = oradrv.Oracle(fa)
    c["by_name"] = {b.name: b for b in c["batches"] + [c["big"]]}
    assert sorted(c["by_name"]) == sorted(NAMES)
    c["ora"] = {n: extcases.oracle(c["drv"], b) for n, b in c["by_name"].items()}
    yield c
    c["ref"].close()
    c["drv"].close()
    shutil.rmtree(os.path.dirname(fa), ignore_errors=True)


def test_restatement_reaches_every_edge_and_gives_the_planted_answers(cases):
    n = {name: extcases.check_edges(b, cases["ora"][name]) for name, b in cases["by_name"].items()}
    print("\n[ext cases] cases held per batch:", n)
    assert n["main"] >= 70 and n["big"] >= 3500


def test_case_shapes(cases):
    """What the batches claim to be, over all their reads, from the restatement's rows."""
    main, ora = cases["by_name"]["main"], cases["ora"]["main"]
    sh = np.concatenate([a["sh"] for a in ora["reads"]])
    ca = np.concatenate([a["calls"] for a in ora["reads"]])
    rg = np.concatenate([a["regs"] for a in ora["reads"]])
    assert [len(r["chains"]) for r in main.reads][0] == 0 and len(main.reads[-1]["chains"]) == 0 and any(len(r["chains"]) == 0 for r in main.reads[1:-1])
    clamp = sh[:, SH["clamp"]]
    assert all((clamp & bit).any() for bit in (1, 2, 4, 8)), sorted(set(int(x) for x in clamp))     # zero, l_pac, 2 * l_pac, an inner contig boundary
    L = main.L
    t0 = ca[ca[:, CL["tlen"]] == 0]
    strand_of = np.array([int(main.reads[i]["sd"][0, 0] >= L) for i, a in enumerate(ora["reads"]) for _ in range(len(a["calls"]))])
    assert {(int(s), int(st)) for s, st in zip(t0[:, CL["side"]], strand_of[ca[:, CL["tlen"]] == 0])} == {(0, 0), (0, 1), (1, 0), (1, 1)}   # tlen == 0 on both sides, both strands
    assert (t0[:, CL["score"]] == t0[:, CL["h0"]]).all() and (t0[:, CL["gscore"]] == -1).all() and (t0[:, CL["qle"]] == 0).all()
    assert sh[:, SH["tlen_short"]].sum() >= 1
    assert sh[:, SH["band2_left"]].sum() == 2 and sh[:, SH["band2_right"]].sum() == 2 and (rg[:, extcases.RG["w"]] == 200).sum() == 4
    assert sh[:, SH["toend_left"]].sum() >= 3 and sh[:, SH["toend_right"]].sum() >= 4
    assert sh[:, SH["skipped"]].sum() >= 5 and sh[:, SH["kept_overlap"]].sum() == 1
    for side in (0, 1):
        assert {31, 32, 47, 48, 63, 64, 95, 96, 127, 128, 159, 160, 249} <= set(int(x) for x in ca[ca[:, CL["side"]] == side, CL["qlen"]])
    assert sorted(set(extcases.ext_class(int(x)) for x in ca[:, CL["qlen"]])) == list(range(7))
    w = extcases.first_wavefront(main, ora)
    assert w["classes"] == list(range(7)) and w["wait"] >= 5 and w["finish"] >= 1 and w["empty"] == 3, w   # one wavefront: all seven class ballots, lanes that wait, finish, return
    assert len(ora["rows"]["chains"]) > 64
    nodp = cases["ora"]["no DP"]
    assert sum(len(a["calls"]) for a in nodp["reads"]) == 0 and len(nodp["rows"]["chains"]) == 2
    for n in (63, 64, 65):
        o = cases["ora"][f"active={n}"]
        assert len(o["rows"]["chains"]) == n and all(len(a["calls"]) == 2 for a in o["reads"])
    assert 4100 <= len(cases["ora"]["big"]["rows"]["chains"]) < 4110


def test_entry_points_refuse_what_the_reference_would_not_accept(cases):
    o, g = cases["drv"], cases["genome"]
    L = int(g.off[-1])
    read = g.seqs[0][1000:1150]
    ok_ch, ok_sd = [[1040, 0, 1, 0, 30, 3, -1, 0]], [[1040, 40, 30, 30]]
    assert o.chain2aln(read, ok_ch, ok_sd) is not None
    bad = [(ok_ch, [[1040, 40, 0, 0]]), (ok_ch, [[1040, -1, 30, 30]]), (ok_ch, [[1040, 130, 30, 30]]), (ok_ch, [[1040, 40, 30, 29]]),
           ([[1040, 1, 1, 0, 30, 3, -1, 0]], ok_sd),                                     # rid is not the seed's contig
           ([[1040, 3, 1, 0, 30, 3, -1, 0]], ok_sd), ([[1040, -1, 1, 0, 30, 3, -1, 0]], ok_sd),
           (ok_ch, [[int(g.off[1]) - 10, 40, 30, 30]]),                                  # a seed across a contig boundary
           (ok_ch, [[L - 10, 40, 30, 30]]), (ok_ch, [[2 * L - 10, 40, 30, 30]]), (ok_ch, [[-5, 40, 30, 30]]),
           ([[1040, 0, 2, 0, 60, 3, -1, 0]], [[1040, 40, 30, 30], [2 * L - 2000, 80, 30, 30]]),   # one chain on two strands
           ([[1040, 0, 2, 0, 30, 3, -1, 0]], ok_sd)]                                     # more seeds than rows
    for ch, sd in bad:
        assert o.chain2aln(read, ch, sd) is None, (ch, sd)
        with pytest.raises(api.ArachneError, match="code -2"):
            api.selftest_ext_stage(cases["ref"], read, [150], [len(ch)], ch, [len(sd)], sd, [0])
    with pytest.raises(api.ArachneError, match="code -2"):                               # two chains on the same seed rows
        api.selftest_ext_stage(cases["ref"], read, [150], [2], ok_ch + ok_ch, [1], ok_sd, [0])
    with pytest.raises(api.ArachneError, match="code -2"):
        api.selftest_ext_stage(cases["ref"], np.full(150, 5, dtype=np.uint8), [150], [1], ok_ch, [1], ok_sd, [0])


@pytest.mark.parametrize("closed", [0, 1])
@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_host_double_against_the_restatement(cases, name, order, closed, monkeypatch):
    monkeypatch.setenv("ARX_EXT_CLOSED", str(closed))
    b, ora = cases["by_name"][name], cases["ora"][name]
    dev = extcases.run_device(cases["ref"], b, ora, order=order)
    n = extcases.check_device(b, ora, dev, bool(closed))
    if name == "no DP":                         # the round loop's `nt == 0` continue: a round with a chain still active and no task
        assert dev["rounds"].tolist() == [[2, 1] + [0] * 7, [3, 0] + [0] * 7] and dev["ext_rounds"] == 0 and dev["done_round"].tolist() == [2, 3]
    if order == 0:
        print(f"\n[ext cases] {name}, closed form {closed}: {n}, {dev['n_ext_tasks']} tasks in {dev['ext_rounds']} rounds")

"""The planted extension-stage cases (tests/extcases.py; tests/test_ext_cases_hostsim.py holds the restatement to their hand-written answers) through
libarachne_amd.so's arx_selftest_ext_stage: Pipeline<HipRT>::stage_extend itself -- KExtInit, KExtStep with its ballots and its seven class lists,
the round loop over the double-buffered active lists, run_extend in each of its launch forms, KExtGather, KDedup -- on chains and seeds written
directly.  Everything is compared with the restatement without a tolerance (extcases.check_device): the gathered regions bit for bit with
ora_chain2aln's rows, the core regions with mem_sort_dedup_patch on those rows, the task count and the census's class totals with the call list,
every chain's n_regs with its shape row, and every dependent chain finishes in a later round than the chain it waited for.

The forms: the launch shapes of arx_batch_run, every launch on ONE workgroup (grid_cap = 1: each lane strides through up to 65 chains of the big
batch), ARX_WIDE=0, run_extend's per-class launches (ARX_EXT_MERGE=0), its merged launch, ARX_EXT_OLD=1 and the one-thread path (ARX_SW_SIMPLE), the
closed form off and on, and a second call in one process.  One call of the entry per test, except the second-call tests (two): each call makes a
runtime of its own, which is what a test costs (profiles/ext_stage/README.md)."""
import os
import shutil
import time

import pytest

import extcases
import oradrv
from arachne_amd import api

pytestmark = pytest.mark.gpu

NAMES = ["main", "no DP", "active=63", "active=64", "active=65", "big"]
SWITCHES = ("ARX_WIDE", "ARX_EXT_MERGE", "ARX_EXT_OLD", "ARX_SW_SIMPLE", "ARX_EXT_CLOSED")
LAUNCH_FORMS = {"per class": {"ARX_EXT_MERGE": "0"}, "merged": {"ARX_EXT_MERGE": "1000000000"}, "old per class": {"ARX_EXT_MERGE": "0", "ARX_EXT_OLD": "1"},
                "old merged": {"ARX_EXT_MERGE": "1000000000", "ARX_EXT_OLD": "1"}, "simple": {"ARX_SW_SIMPLE": "1"}}


@pytest.fixture(scope="module")
def cases(built):
    c = extcases.build_all()
    fa = c["genome"].write_index()
    c["ref"] = api.Reference(fa)
    c["drv"] = oradrv.Oracle(fa)
    c["by_name"] = {b.name: b for b in c["batches"] + [c["big"]]}
    assert sorted(c["by_name"]) == sorted(NAMES)
    c["ora"] = {}
    for n, b in c["by_name"].items():
        c["ora"][n] = extcases.oracle(c["drv"], b)
        extcases.check_edges(b, c["ora"][n])          # every case shows its edge before the device is looked at
    w = extcases.first_wavefront(c["by_name"]["main"], c["ora"]["main"])
    assert w["classes"] == list(range(7)) and w["wait"] >= 5 and w["finish"] >= 1 and w["empty"] == 3, w
    yield c
    c["ref"].close()
    c["drv"].close()
    shutil.rmtree(os.path.dirname(fa), ignore_errors=True)


def _run(cases, name, what, monkeypatch, env=None, closed=True, **kw):
    for k in SWITCHES:                                # the switches are read when the entry makes its runtime and its pipeline
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if not closed:
        monkeypatch.setenv("ARX_EXT_CLOSED", "0")
    b, ora = cases["by_name"][name], cases["ora"][name]
    t0 = time.time()
    dev = extcases.run_device(cases["ref"], b, ora, **kw)
    dt = time.time() - t0
    n = extcases.check_device(b, ora, dev, closed)
    print(f"\n[ext stage gpu] {what}, {name}: {dt:.2f} s, {len(b.reads)} reads, {n['chains']} chains, {n['calls']} calls, {dev['n_ext_tasks']} tasks in "
          f"{dev['ext_rounds']} of {n['rounds']} rounds, {n['regions']} regions, {n['core']} after de-duplication")
    if name == "no DP":                               # the round loop's `nt == 0` continue: a round with a chain still active and no task
        assert dev["rounds"].tolist() == [[2, 1] + [0] * 7, [3, 0] + [0] * 7] and dev["ext_rounds"] == 0 and dev["done_round"].tolist() == [2, 3]
    return dev


@pytest.mark.parametrize("name", NAMES)
def test_default(cases, name, monkeypatch):
    _run(cases, name, "default", monkeypatch)


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_off(cases, name, monkeypatch):
    _run(cases, name, "ARX_EXT_CLOSED=0", monkeypatch, closed=False)


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_one_workgroup(cases, name, closed, monkeypatch):
    _run(cases, name, f"grid_cap 1, closed form {int(closed)}", monkeypatch, closed=closed, grid_cap=1)


@pytest.mark.parametrize("name", ["main", "active=65", "big"])
def test_wide_off(cases, name, monkeypatch):
    _run(cases, name, "ARX_WIDE=0", monkeypatch, env={"ARX_WIDE": "0"}, closed=False)


@pytest.mark.parametrize("grid_cap", [0, 1])
@pytest.mark.parametrize("form", sorted(LAUNCH_FORMS))
@pytest.mark.parametrize("name", ["main", "big"])
def test_launch_forms_of_run_extend(cases, name, form, grid_cap, monkeypatch):
    _run(cases, name, f"{form}, grid_cap {grid_cap}", monkeypatch, env=LAUNCH_FORMS[form], closed=False, grid_cap=grid_cap)


@pytest.mark.parametrize("name", ["main", "big"])
def test_second_call_in_one_process(cases, name, monkeypatch):
    a = _run(cases, name, "first of two", monkeypatch)
    b = _run(cases, name, "second of two", monkeypatch)
    for k in ("ext_off", "ext_regs", "core_off", "core_regs", "core_clean", "rounds", "done_round", "n_regs"):
        assert a[k].tobytes() == b[k].tobytes(), k                                      # nothing of a call is left for the next

"""The planted post-pass cases (tests/postcases.py; tests/test_post_cases_hostsim.py holds the restatement to their hand-written answers) through
libarachne_amd.so's arx_selftest_post: PostStage<HipRT>::run itself -- post_walk, the scan, post_fill, post_active, dup_insert, dup_mark, split --
on candidates written directly.  Every record, both mismatch lists and every split field are compared with ora_post bit for bit, in the launch
shapes of arx_batch_post, with every launch on ONE workgroup (grid_cap = 1: each lane strides through up to 128 items) and with ARX_WIDE=0 (the
capped grid-stride form of launch_wide).  The census -- the duplicate table as dup_insert's compare-and-swap and atomic minimum left it, and every
read's home slot -- must show one slot per key holding the group's first read, whatever order the lanes arrived in.

One call of the entry per test: each call makes a runtime of its own, which is what a test costs (profiles/post_stage/README.md)."""
import os
import shutil
import time

import numpy as np
import pytest

import oradrv
import postcases
from arachne_amd import api

pytestmark = pytest.mark.gpu

NAMES = ["walk", "candidates=63", "candidates=64", "candidates=65", "placeholders only", "duplicate groups", "split", "probe R=32", "probe R=34",
         "same home", "duplicate group of 4096", "probe R=2048"]
CAPS = {"same home": 64, "probe R=32": 64, "probe R=34": 128, "probe R=2048": 4096, "duplicate group of 4096": 16384}


@pytest.fixture(scope="module")
def cases(built):
    c = postcases.build_all()
    fa = c["genome"].write_index()
    c["ref"] = api.Reference(fa)
    c["drv"] = oradrv.Oracle(fa)
    c["by_name"] = {f["name"]: f for f in c["batches"] + c["big"]}
    assert sorted(c["by_name"]) == sorted(NAMES)
    for f in c["by_name"].values():
        f["ora"] = postcases.oracle(c["drv"].h, f)
        postcases.check_expected(f, f["ora"])
    yield c
    c["ref"].close()
    c["drv"].close()
    shutil.rmtree(os.path.dirname(fa), ignore_errors=True)


def _run(cases, name, what, **kw):
    f = cases["by_name"][name]
    t0 = time.time()
    dev = postcases.run_device(cases["ref"], f, census=True, **kw)
    print(f"\n[post stage gpu] {what}, {name}: {time.time() - t0:.2f} s, {f['n_reads']} reads, {len(f['cands'])} candidates, {len(dev['mm_ref'])} locations")
    postcases.check_device(dev, f["ora"])
    cen = postcases.check_census(f, dev)
    if name in CAPS:
        assert cen["cap"] == CAPS[name]
    if name == "probe R=32":
        assert cen["shared_home_in_run"] and cen["longest"] >= 4
    if name == "probe R=2048":
        assert cen["wrapped"]
    return dev


@pytest.mark.parametrize("name", NAMES)
def test_default(cases, name, monkeypatch):
    monkeypatch.delenv("ARX_WIDE", raising=False)
    _run(cases, name, "default")


@pytest.mark.parametrize("name", NAMES)
def test_one_workgroup(cases, name):
    _run(cases, name, "grid_cap 1", grid_cap=1)


@pytest.mark.parametrize("name", NAMES)
def test_wide_off(cases, name, monkeypatch):
    monkeypatch.setenv("ARX_WIDE", "0")
    _run(cases, name, "ARX_WIDE=0")


def test_split_without_centromere_arrays(cases):
    f = cases["by_name"]["split"]
    ora = postcases.oracle(cases["drv"].h, f, centromeres=None)
    assert postcases.check_expected(f, ora, with_centromeres=False) == len(f["split"])
    postcases.check_device(postcases.run_device(cases["ref"], f, centromeres=None), ora)


@pytest.mark.parametrize("name", ["duplicate group of 4096", "probe R=2048"])
def test_second_call_in_one_process(cases, name):
    a = _run(cases, name, "first of two")
    b = _run(cases, name, "second of two")
    for k in ("post", "split", "mm_ref", "mm_read", "home"):
        assert a[k].tobytes() == b[k].tobytes(), k                                      # nothing of a call is left for the next
    assert np.array_equal(np.sort(a["table"]), np.sort(b["table"]))                     # (which of two colliding keys took which slot may differ)

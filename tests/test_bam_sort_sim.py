"""CPU test of the coordinate sort's device logic (arachne_amd/csrc/dev_bamsort.h): tests/sortsim/bam_sort_sim.cpp compiles the very functions
the kernels run, with the items of a launch in a loop, under -fsanitize=address,undefined, and is run as a plain process.  Every stream goes in
from an allocation of exactly its size; every case runs at seg_bytes 64, 256 and 4096 with the items in ascending and in descending order
(the program holds the six runs to one another); output bytes, record offsets and record count are compared with what sortcases.py took from
Python's stable sorted().  Also here, needing no GPU either: arx_bam_open_ex with a NULL context against arx_bam_open."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reccases
import sortcases as sc
from arachne_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sortsim") / "bam_sort_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "sortsim", "bam_sort_sim.cpp"), "-o", exe])
    return exe


def _run(sim, tmp, stream, n_ref, slab=None):
    """-> (status, records, [(seg, rev, segments, right, repaired, rounds)], rec_off, output bytes)"""
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(stream)
    if os.path.exists(dst):
        os.remove(dst)
    r = subprocess.run([sim, "copy" if slab else "sort", src, dst, str(n_ref)] + ([str(slab)] if slab else []), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    status, records = int(lines[0].split()[1]), int(lines[1].split()[1])
    cfg = [tuple(int(x) for x in l.split()[1:]) for l in lines[2:8]]
    assert [(c[0], c[1]) for c in cfg] == [(g, v) for g in sc.SEGS for v in (0, 1)]
    rec_off = [int(x) for x in lines[8].split()[1:]]
    out = open(dst, "rb").read() if os.path.exists(dst) else None
    return status, records, cfg, rec_off, out


def test_the_cases_are_what_they_claim():
    sc.check_cases()


@pytest.mark.parametrize("name", list(sc.cases()))
def test_sort(sim, tmp_path, name):
    case = sc.cases()[name]
    status, records, cfg, rec_off, out = _run(sim, str(tmp_path), case.stream, case.n_ref)
    assert status == 0 and records == case.n
    assert out == case.out
    assert rec_off == case.rec_off.tolist()
    for seg, rev, segments, right, repaired, rounds in cfg:
        assert segments == -(-len(case.stream) // seg) and right + repaired == max(segments - 1, 0) and rounds <= segments
    if name == "decoy":
        assert all(c[4] >= 1 for c in cfg), cfg              # the fake chain was the guess, and was walked again


@pytest.mark.parametrize("name", list(sc.broken()))
def test_broken_chains_are_refused_and_nothing_is_written(sim, tmp_path, name):
    s = sc.broken()[name]
    status, records, cfg, rec_off, out = _run(sim, str(tmp_path), s, sc.N_REF)
    assert status == 1 and out == b"\xa5" * len(s) and rec_off == []
    assert _run(sim, str(tmp_path), s, sc.N_REF, slab=50)[0] == 1


@pytest.mark.parametrize("slab", [37, 50, 333, 5000])
def test_copy_mode_counts_over_slabs_cut_inside_records(sim, tmp_path, slab):
    for name in ("one_minimal", "start_on_border", "spans_segments", "name_lengths", "decoy", "unmapped_scattered"):
        case = sc.cases()[name]
        assert any(0 < (int(o) % slab) for o in case.in_off[1:-1]) or case.n < 2          # slabs end inside records
        status, records, cfg, _, _ = _run(sim, str(tmp_path), case.stream, case.n_ref, slab=slab)
        assert status == 0 and records == case.n, (name, slab)


def _header_text(path):
    data = reccases.inflate(path)
    return data, data[8:8 + int.from_bytes(data[4:8], "little")]


def test_open_ex_without_a_context_is_open(tmp_path):
    lib = api._load(api.LIB_PATH)
    names, lens = ["chrA", "chrB"], np.array([1000, 2000], dtype=np.int32)
    recs = sc.cases()["unmapped_scattered"]
    files = {}
    for tag, flags in (("old", None), ("ex0", 0), ("ex1", 1)):
        p = str(tmp_path / (tag + ".bam"))
        w = api.BamWriter(p, names, lens, extra_header="@PG\tID:t\n", threads=2, level=1, **({} if flags is None else {"flags": flags}))
        w.write_encoded(recs.stream, recs.n)
        w.close()
        files[tag] = open(p, "rb").read()
    assert files["old"] == files["ex0"]                                    # flags = 0: byte for byte the existing call's file
    d0, t0 = _header_text(str(tmp_path / "ex0.bam"))
    d1, t1 = _header_text(str(tmp_path / "ex1.bam"))
    assert t0.startswith(b"@HD\tVN:1.6\tSO:unknown\n") and t1 == t0.replace(b"SO:unknown", b"SO:coordinate", 1)
    assert d1[:4] == d0[:4] and d1[8 + len(t1):] == d0[8 + len(t0):]      # only the SO value differs (and with it l_text)
    h = C.c_void_p()
    msg = C.create_string_buffer(256)
    fn = api._selftest_fn(lib, "arx_bam_open_ex")
    c_names = (C.c_char_p * 2)(b"chrA", b"chrB")
    assert fn(None, str(tmp_path / "bad.bam").encode(), 2, c_names, lens.ctypes.data, None, 1, 1, 2, C.byref(h), msg, 256) == api.ARX_E_ARG    # an unknown bit
    assert not h.value and b"flag" in msg.value

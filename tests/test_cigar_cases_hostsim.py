"""The planted CIGAR-stage cases (tests/cigarcases.py) on the CPU.

First the cases are held to what they claim, from the restatement's shape rows alone (oracle/arx_oracle.c ora_reg2aln): the gap-free rule on
both sides of its edge, every first-band class at its n_col edge, one, two and three bwa_gen_cigar2 calls with each reason to stop, punts, the
squeeze of a leading or trailing deletion, the clips, CIGAR slots at their limit, contig edges, long regions.  Then the restatement is held to the
compiled reference (mem_reg2aln, where oracle/_ref exists) field for field, and the host double's arx_selftest_reg2aln -- Pipeline::stage_reg2aln
with the serial reg2aln of dev_regs.h behind it -- to the restatement, with its census.  tests/test_cigar_stage_gpu.py runs the same batches on the GPU.

Two conditions cannot be met by any input, by arithmetic, and are asserted as such: a SECOND call never leaves its class kernel's tilings (the
band doubles once, HI is the doubled tiling), so punts are third calls; and class 3 (HI = 16 columns per lane, 256 in all) never punts because
n_col <= l1 <= 255."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cigarcases as cc
import oradrv
import refdrv
from arachne_amd import api

SIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "libarx_hostsim.so")
F = {n: i for i, n in enumerate(oradrv.Oracle.R2A_FIELDS)}


@pytest.fixture(scope="module")
def cases(built):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    main, small = cc.build_main(), cc.build_small()
    c = dict(main=main, small=small)
    for name, b in (("main", main), ("small", small)):
        fa = cc.write_index(b, lib_path=SIM)
        o = oradrv.Oracle(fa)
        flat = cc.flatten(b)
        c[name + "_fa"], c[name + "_flat"], c[name + "_exp"] = fa, flat, cc.expected(o, flat)
        c[name + "_ora"] = o
    c["ref"] = api.Reference(c["main_fa"], lib_path=SIM)
    c["ref_small"] = api.Reference(c["small_fa"], lib_path=SIM)
    yield c
    c["ref"].close(); c["ref_small"].close()
    c["main_ora"].close(); c["small_ora"].close()
    for name in ("main", "small"):
        shutil.rmtree(os.path.dirname(c[name + "_fa"]), ignore_errors=True)


def _sel(flat, exp, pred):
    sh, a, rows = exp["shapes"], exp["alns"], flat["rows"]
    return [g for g in range(len(rows)) if pred(sh[g], a[g], rows[g], flat["tags"][g])]


def _strands(flat, exp, pred, what):
    """The condition holds for a region on each strand."""
    hits = _sel(flat, exp, pred)
    rev = {int(exp["alns"][g, 3]) for g in hits}
    assert rev == {0, 1}, f"{what}: strands {sorted(rev)} ({len(hits)} regions)"
    return hits


def _cigar(exp, g):
    a = exp["alns"][g]
    return [(int(x) >> 4, int(x) & 15) for x in exp["cigars"][a[8]:a[8] + a[7]]]


def test_shape_gapfree_rule(cases):
    flat, exp = cases["main_flat"], cases["main_exp"]
    l1 = lambda r: r[cc.COL["qe"]] - r[cc.COL["qb"]]
    l2 = lambda r: r[cc.COL["re"]] - r[cc.COL["rb"]]
    _strands(flat, exp, lambda s, a, r, t: l1(r) == l2(r) and l1(r) - r[cc.COL["truesc"]] == 11 and s[F["w_0"]] == 0 and s[F["calls"]] == 1, "loss 11 is gap-free")
    _strands(flat, exp, lambda s, a, r, t: l1(r) == l2(r) and l1(r) - r[cc.COL["truesc"]] == 12 and s[F["w_0"]] == 8, "loss 12 is queued with band 8")
    _strands(flat, exp, lambda s, a, r, t: l1(r) != l2(r) and min(l1(r), l2(r)) == r[cc.COL["truesc"]] and s[F["w0"]] > 0, "unequal lengths with loss 0 are queued")
    _strands(flat, exp, lambda s, a, r, t: l1(r) == l2(r) and l1(r) - r[cc.COL["truesc"]] < 12 and s[F["calls"]] == 2 and s[F["stop"]] == 1 and s[F["w_1"]] == 0,
             "a gap-free region called twice, stopped by the equal score")
    # queued (the rule says gapped) and still the shortcut inside bwa_gen_cigar2: the row's w clamps the band to 0
    _strands(flat, exp, lambda s, a, r, t: l1(r) == l2(r) and l1(r) - r[cc.COL["truesc"]] >= 12 and s[F["w_0"]] == 0 and s[F["w0"]] == -1, "queued region that takes the shortcut")


def test_shape_classes(cases):
    flat, exp = cases["main_flat"], cases["main_exp"]
    want = cc.census_from_shapes(flat, exp["shapes"])
    q = want["queued"]
    for n in (16, 17, 32, 33, 64, 65, 128, 129):
        _strands(flat, exp, lambda s, a, r, t: q[_g(flat, r)] and s[F["n_col0"]] == n, f"first band of {n} columns")
    _strands(flat, exp, lambda s, a, r, t: s[F["n_col0"]] >= 200, "first band of 200 columns and more")
    for n in (15, 31, 63, 127):   # and the odd widths 2 w + 1 next to each edge
        _strands(flat, exp, lambda s, a, r, t: s[F["n_col0"]] == n, f"first band of {n} columns")
    assert max(want["per_class"]) >= 65 and min(want["per_class"]) >= 5, want["per_class"]
    # lists of 1, 3, 4 and 5 regions (a partial, a full and a spilling wavefront of four groups): the small batch
    small = cc.census_from_shapes(cases["small_flat"], cases["small_exp"]["shapes"])
    assert small["per_class"][:4] == [1, 3, 4, 5], small["per_class"]
    assert int(small["punt"].sum()) == 0 and int(want["punt"].sum()) >= 20


def _g(flat, row):
    return int(np.flatnonzero((flat["rows"] == row).all(axis=1))[0])


def test_shape_retries(cases):
    flat, exp = cases["main_flat"], cases["main_exp"]
    want = cc.census_from_shapes(flat, exp["shapes"])
    for n in (1, 2, 3):
        _strands(flat, exp, lambda s, a, r, t: s[F["calls"]] == n and s[F["w0"]] > 0, f"{n} calls")
        _strands(flat, exp, lambda s, a, r, t: s[F["calls"]] == n and s[F["stop"]] & 2 and s[F["w_0"] + n - 1] == 400, f"the band cap reached at call {n}")
    _strands(flat, exp, lambda s, a, r, t: s[F["stop"]] == 1 and s[F["w0"]] > 0, "stop on an equal score")
    _strands(flat, exp, lambda s, a, r, t: s[F["calls"]] == 3 and s[F["stop"]] == 0 and len({s[F["score0"]], s[F["score1"]], s[F["score2"]]}) == 3, "three calls, three scores")
    m = lambda r: min(r[cc.COL["qe"]] - r[cc.COL["qb"]], r[cc.COL["re"]] - r[cc.COL["rb"]])
    _strands(flat, exp, lambda s, a, r, t: 100 < r[cc.COL["w"]] < m(r) - r[cc.COL["truesc"]] - 4 and s[F["w_0"]] == r[cc.COL["w"]], "w0 > 100 cut down to the row's w")
    _strands(flat, exp, lambda s, a, r, t: 100 < m(r) - r[cc.COL["truesc"]] - 4 < r[cc.COL["w"]] and s[F["w_0"]] == m(r) - r[cc.COL["truesc"]] - 4, "w0 > 100 below the row's w")
    hi = [32, 64, 128, 256]
    for c in range(4):
        inside = [g for g in np.flatnonzero(want["queued"] & (want["klass"] == c)) if exp["shapes"][g, F["calls"]] >= 2 and exp["shapes"][g, F["n_col1"]] <= hi[c]
                  and exp["shapes"][g, F["n_col1"]] > exp["shapes"][g, F["n_col0"]]]
        assert {int(exp["alns"][g, 3]) for g in inside} == {0, 1}, f"class {c}: a second, wider try inside the class kernel's tilings"
        p3 = [g for g in np.flatnonzero(want["punt"] & (want["klass"] == c)) if exp["shapes"][g, F["n_col2"]] > hi[c] >= exp["shapes"][g, F["n_col1"]]]
        if c < 3:
            assert {int(exp["alns"][g, 3]) for g in p3} == {0, 1}, f"class {c}: a third try that punts where the second did not"
    # by arithmetic (module docstring): no second try punts, class 3 and 4 never do
    sh = exp["shapes"]
    qd = want["queued"]
    assert not (qd & (sh[:, F["n_col1"]] > np.array(hi + [256])[want["klass"]])).any()
    assert not (want["punt"] & (want["klass"] >= 3)).any()


def test_band_cap_cannot_show(cases):
    """Why no case can tell a cap of 200 from the cap of 400 (profiles/cigar_stage: mutation 7): bwa_gen_cigar2 limits the band to
    (max_gap + d + 1) >> 1 <= 121 or fixes it at d + 3, so from w_ = 122 on the band no longer depends on w_.  Held here on every case: an
    executed call with w_ >= 200 runs the band that w_ = 200 gives, and where the call before it had w_ >= 122 it repeats that call's band,
    columns and score (so a call more or a call less at the capped band changes no record)."""
    seen = 0
    for name in ("main", "small"):
        flat, sh = cases[name + "_flat"], cases[name + "_exp"]["shapes"]
        for g in range(len(sh)):
            r = flat["rows"][g]
            l1, l2 = int(r[3] - r[2]), int(r[1] - r[0])
            d, max_gap = abs(l2 - l1), max(1, ((l1 + 1) >> 1) - 5)
            for i in range(int(sh[g, F["calls"]])):
                if sh[g, F["w_0"] + i] < 200:
                    continue
                seen += 1
                if i > 0 and sh[g, F["w_0"] + i - 1] >= 122:
                    assert all(sh[g, F[c] + i] == sh[g, F[c] + i - 1] for c in ("w0", "n_col0", "score0")), (name, g, i)
                assert sh[g, F["w0"] + i] == max(min((max_gap + d + 1) >> 1, 200), d + 3), (name, g, i)
    assert seen >= 10


def test_shape_slices(cases):
    flat, exp = cases["main_flat"], cases["main_exp"]
    want = cc.census_from_shapes(flat, exp["shapes"])
    rows, sh = flat["rows"], exp["shapes"]
    l2 = rows[:, cc.COL["re"]] - rows[:, cc.COL["rb"]]
    # the last try runs at the band the slice is sized for: bwa_gen_cigar2 caps w at (max_gap + d + 1) >> 1 = 62 for 255 x 255, so no wider try exists
    full = [int(g) for g in np.flatnonzero(want["queued"] & (want["klass"] == 3) & (l2 >= 200))
            if sh[g, F["w0"] + sh[g, F["calls"]] - 1] == 62 and 16 * cc.tiling(int(sh[g, F["n_col0"] + sh[g, F["calls"]] - 1])) * l2[g] == want["need_bytes"][g]]
    run = best = 1
    for a, b in zip(full, full[1:]):   # next to each other in the batch, hence in the queue of one class launch
        run = run + 1 if b == a + 1 else 1
        best = max(best, run)
    assert best >= 30, (len(full), best)


def test_shape_squeeze_and_clips(cases):
    flat, exp = cases["main_flat"], cases["main_exp"]
    def squeezed_len(g):   # reference bases of the region that the final CIGAR no longer covers
        r = flat["rows"][g]
        return int(r[1] - r[0]) - sum(n for n, op in _cigar(exp, g) if op in (0, 2))
    for n, ok in ((1, lambda k: k == 1), (10, lambda k: k >= 10)):
        for g in _strands(flat, exp, lambda s, a, r, t: s[F["squeezed"]] == 1 and s[F["core_n"]] == 2 and ok(squeezed_len(_g(flat, r))), f"leading deletion of {n}"):
            r, a = flat["rows"][g], exp["alns"][g]
            assert a[6] == 0   # not counted in NM
            if not a[3]:       # pos moved by its length
                assert a[0] + cases["main"].off[a[1]] == r[0] + squeezed_len(g)
    for g in _strands(flat, exp, lambda s, a, r, t: s[F["squeezed"]] == 2, "trailing deletion squeezed"):
        assert exp["alns"][g, 6] == 0 and _cigar(exp, g)[-1][1] != 2
    both = _strands(flat, exp, lambda s, a, r, t: s[F["squeezed"]] == 1 and t.startswith("lead and trail"), "leading and trailing deletion at once")
    for g in both:
        cg = _cigar(exp, g)
        assert [op for _, op in cg] == [3, 0, 2, 3] and exp["alns"][g, 6] == 0 and exp["shapes"][g, F["core_n"]] == 3, cg   # the trailing D stays, NM counts neither
    for g in _strands(flat, exp, lambda s, a, r, t: t.startswith("interior D"), "interior deletion"):
        assert [op for _, op in _cigar(exp, g)] == [0, 2, 0] and exp["shapes"][g, F["squeezed"]] == 0 and exp["alns"][g, 6] == 7
    for g in _strands(flat, exp, lambda s, a, r, t: t.startswith("lead I"), "leading insertion"):
        assert _cigar(exp, g)[0][1] == 1 and exp["shapes"][g, F["squeezed"]] == 0
    for c5, c3 in ((0, 0), (1, 0), (0, 1), (1, 1)):
        _strands(flat, exp, lambda s, a, r, t: (s[F["clip5"]] > 0, s[F["clip3"]] > 0) == (bool(c5), bool(c3)) and s[F["w0"]] > 0, f"clips {c5}/{c3}")
    # reverse strand: the clips swap sides (clip5 is what follows qe in the read as given)
    for g in _sel(flat, exp, lambda s, a, r, t: t.startswith("clip 5'")):
        r, l = flat["rows"][g], flat["lens"][flat["read_of"][g]]
        assert exp["shapes"][g, F["clip5"]] == (l - r[cc.COL["qe"]] if exp["alns"][g, 3] else r[cc.COL["qb"]]) == 11 and exp["shapes"][g, F["clip3"]] == 0


def test_shape_slots(cases):
    flat, exp = cases["main_flat"], cases["main_exp"]
    hits = _strands(flat, exp, lambda s, a, r, t: s[F["core_n"]] == 14 and s[F["clip5"]] > 0 and s[F["clip3"]] > 0 and s[F["squeezed"]] == 0, "14 operations and both clips")
    assert all(exp["alns"][g, 7] == 16 for g in hits)
    hits = _strands(flat, exp, lambda s, a, r, t: s[F["core_n"]] == 14 and s[F["squeezed"]] == 1, "a leading deletion squeezed from a CIGAR at the limit")
    for n in (13, 15, 30, 31):
        _strands(flat, exp, lambda s, a, r, t: s[F["core_n"]] == n and s[F["w0"]] > 0 and s[F["n_col0"]] < 64, f"{n} operations")
    core = exp["shapes"][:, F["core_n"]]
    assert core.max() <= 62, "no region may need more than the third pass's 64 words"   # (the junk regions hold 40 to 50 operations)
    nov = cc.flatten(cases["main"], _without_overflow(cases))
    sub = _subset(cases, nov)
    assert sub["shapes"][:, F["max_n"]].max() <= 14 and cc.slot_loop(sub["shapes"]) == (1, 16), "the batch without its overflow cases must fit 16-word slots"
    assert cc.slot_loop(exp["shapes"]) == (3, 64)
    assert len(sub["alns"]) >= len(exp["alns"]) // 2


def _without_overflow(cases):
    return cc.reads_without_overflow(cases["main_flat"], cases["main_exp"]["shapes"])


def _subset(cases, sub):
    return cc.subset(cases["main_flat"], cases["main_exp"], sub)


def test_shape_geometry_and_reads(cases):
    flat, exp, b = cases["main_flat"], cases["main_exp"], cases["main"]
    rows, L = flat["rows"], b.L
    assert (rows[:, 0] == 0).any() and (rows[:, 1] == L).any() and (rows[:, 0] == L).any() and (rows[:, 1] == 2 * L).any()
    ends = set()
    for c in (0, len(cc.CONTIG_LENS) - 1):
        for g in range(len(rows)):
            rb, re = int(rows[g, 0]), int(rows[g, 1])
            if rb >= L:
                rb, re = 2 * L - re, 2 * L - rb
            if rb == b.off[c]:
                ends.add((c, "start", int(exp["alns"][g, 3])))
            if re == b.off[c + 1]:
                ends.add((c, "end", int(exp["alns"][g, 3])))
    assert len(ends) == 8, sorted(ends)
    _strands(flat, exp, lambda s, a, r, t: s[F["squeezed"]] == 1 and a[0] == 9 and t.startswith("lead D at contig start"), "leading deletion squeezed at a contig start")
    cap, n = flat["cap"], flat["n_regs"]
    assert cap[0] == 0 and cap[-1] == 0 and (cap[1:-1] == 0).any() and (n < cap).any() and (n > 1).any()
    lens = flat["lens"]
    assert lens.min() == 30 and lens.max() == 255 and np.count_nonzero(lens == 255) < len(lens) // 2
    assert (rows[:, cc.COL["secondary"]] >= 0).any() and (rows[:, cc.COL["sub"]] < rows[:, cc.COL["csub"]]).any() and (rows[:, cc.COL["sub"]] > rows[:, cc.COL["csub"]]).any()
    assert (rows[:, cc.COL["is_alt"]] == 1).any() and (rows[:, cc.COL["alt_sc"]] > 0).any()
    for g in _strands(flat, exp, lambda s, a, r, t: t.startswith("ambiguous in M"), "ambiguous bases in a match run"):
        assert exp["alns"][g, 6] == 3 and exp["shapes"][g, F["score0"]] == 101 - 2 - 2 - 7 + 1   # two ambiguous bases: NM 2 + the deletion, -1 each (sc_mat)
    l2 = rows[:, 1] - rows[:, 0]
    for n2 in (cc.NW_T_CAP, cc.NW_T_CAP + 1):
        hits = np.flatnonzero(l2 == n2)
        assert {int(exp["alns"][g, 3]) for g in hits} == {0, 1}
        assert all((rows[g, 3] - rows[g, 2]) * n2 <= 255 * (2 * 255 + 64) for g in hits)
    sm = cases["small_flat"]
    sl1, sl2 = sm["rows"][:, 3] - sm["rows"][:, 2], sm["rows"][:, 1] - sm["rows"][:, 0]
    z_cap = int(sm["lens"].max()) * (2 * int(sm["lens"].max()) + 64)
    beyond = np.flatnonzero((sl2 > cc.NW_T_CAP) & (sl1 * sl2 > z_cap))
    assert len(beyond) == 1 and sm["tags"][beyond[0]] == "beyond z_cap" and ((sl2 > cc.NW_T_CAP) & (sl1 * sl2 <= z_cap)).any()


@pytest.mark.parametrize("name", ["main", "small"])
def test_restatement_equals_reference(cases, name):
    refdrv.need("ref_reg2aln")   # (asked after the `built` fixture has had its chance to rebuild the library)
    r = refdrv.Ref(cases[name + "_fa"])
    try:
        ref = cc.expected(r, cases[name + "_flat"], with_shape=False)
    finally:
        r.close()
    exp = cases[name + "_exp"]
    bad = np.argwhere(ref["alns"] != exp["alns"])
    assert len(bad) == 0, f"aln row {bad[0][0]} ({cases[name + '_flat']['tags'][bad[0][0]]}) column {bad[0][1]}: reference {ref['alns'][bad[0][0]]}, restatement {exp['alns'][bad[0][0]]}"
    assert ref["cigars"].shape == exp["cigars"].shape and (ref["cigars"] == exp["cigars"]).all()


def _run(ref, flat, census=True):
    return api.selftest_reg2aln(ref, flat["seqs"], flat["lens"], flat["cap"], flat["n_regs"], flat["regs"], census=census)


KNOWN = 0x7ff & ~(1 << 9)   # what the double says it knows: everything but the punts


def test_double_equals_restatement(cases):
    flat, exp = cases["main_flat"], cases["main_exp"]
    dev = _run(cases["ref"], flat)
    assert dev["err"] == 0
    cc.check_stage(dev, flat, exp)
    assert dev["census"]["known"] == KNOWN and dev["census"]["punts"] == -1
    want = cc.check_census(dev["census"], flat, exp["shapes"], passes=3, cig_w=64, punts=False)
    cc.check_slices(dev["census"], want)


def test_double_without_overflow_block(cases):
    sub = cc.flatten(cases["main"], _without_overflow(cases))
    exp = _subset(cases, sub)
    dev = _run(cases["ref"], sub)
    assert dev["err"] == 0
    cc.check_stage(dev, sub, exp)
    cc.check_census(dev["census"], sub, exp["shapes"], passes=1, cig_w=16, punts=False)


def test_double_in_two_halves(cases):
    b, exp = cases["main"], cases["main_exp"]
    h = len(b.reads) // 2
    parts = [cc.flatten(b, range(0, h)), cc.flatten(b, range(h, len(b.reads)))]
    devs = [_run(cases["ref"], p, census=False) for p in parts]
    n0 = int(devs[0]["reg_off"][-1])
    alns = np.concatenate([d["alns"] for d in devs])
    alns["cigar_off"][n0:] += len(devs[0]["cigars"])
    both = dict(reg_off=np.concatenate([devs[0]["reg_off"], devs[1]["reg_off"][1:] + n0]), alns=alns, cigars=np.concatenate([d["cigars"] for d in devs]))
    cc.check_stage(both, cases["main_flat"], exp)


def test_double_pool_overflow(cases):
    flat, exp = cases["small_flat"], cases["small_exp"]
    dev = _run(cases["ref_small"], flat)
    assert dev["err"] == cc.ERR_POOL_OVERFLOW
    cc.check_stage(dev, flat, exp, skip=[flat["tags"].index("beyond z_cap")])
    want = cc.check_census(dev["census"], flat, exp["shapes"], passes=1, cig_w=16, punts=False)
    cc.check_slices(dev["census"], want)


def test_entry_refuses_what_a_kernel_would_index_with(cases):
    flat = cc.flatten(cases["small"])
    L = cases["small"].L
    g = int(np.flatnonzero((flat["regs"][:, 1] > 0) & (flat["regs"][:, 0] < L))[0])   # a used forward-strand slot
    r = int(np.searchsorted(np.cumsum(flat["cap"]), g, side="right"))

    def bad(**kw):
        regs = flat["regs"].copy()
        lens, cap, n_regs = flat["lens"].copy(), flat["cap"].copy(), flat["n_regs"].copy()
        for k, v in kw.items():
            if k == "n_regs":
                n_regs[r] = v
            else:
                regs[g, cc.COL[k]] = v
        with pytest.raises(api.ArachneError) as e:
            api.selftest_reg2aln(cases["ref_small"], flat["seqs"], lens, cap, n_regs, regs)
        assert e.value.code == api.ARX_E_ARG

    row = flat["regs"][g]
    bad(qb=-1); bad(qe=int(flat["lens"][r]) + 1); bad(qb=int(row[3])); bad(rb=-1); bad(re=int(row[0])); bad(re=L + 5, rb=L - 5); bad(re=2 * L + 1, rb=2 * L - 50)
    bad(w=-1); bad(re=int(row[0]) + 4097); bad(n_regs=int(flat["cap"][r]) + 1); bad(truesc=1 << 25)


def test_double_slot_cases_alone(cases):
    for tag, sub, sexp, passes, cig_w in cc.slot_batches(cases["main"], cases["main_flat"], cases["main_exp"]):
        dev = _run(cases["ref"], sub)
        assert dev["err"] == 0, tag
        cc.check_stage(dev, sub, sexp)
        cc.check_census(dev["census"], sub, sexp["shapes"], passes=passes, cig_w=cig_w, punts=False)

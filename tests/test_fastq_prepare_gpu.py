"""A FASTQ file pair standardized and sorted by barcode in one call on the GPU (arx_fastq_prepare, arx_selftest_fastq_prepare;
arachne_amd/csrc/dev_fqprep.h, hip_fqprep.h).  1. the cases of fqprepcases.py -- the ones tests/test_fastq_prepare_sim.py runs through the host
program -- through the kernels, in core and in runs, held to the two restatements composed; 2. files of every form into plain and BGZF outputs,
in core and through run files; 3. the same outputs against the product's own arx_fastq_standardize followed by arx_fastq_sort_ex, byte for
byte; 4. the property: the host feeder reads every barcode of the output as one set with the restatement's fields; 5. CHECK, a standard pair,
e2e.prepare; 6. what is refused, and that nothing is left behind."""
import ctypes as C
import os

import numpy as np
import pytest

import bgzfio
import devfeed
import fqprepcases as pc
import fqsortcases as fc
import fqstdcases as sc
from arachne_amd import api, e2e
from test_fastq_standardize_gpu import _pairs_of, _read_output, _write_forms

pytestmark = pytest.mark.gpu


def _hold(name, c, r, in_core_or_runs=True):
    st = r["stats"]
    if c.exp is None:                                                        # "auto" found no format: nothing is written
        assert r["rc"] == api.ARX_E_ARG and (st["format"], st["decided_by"]) == ("unknown", -1), name
        assert r["n_records"] == -1 and (r["out_len"] == -1).all() and (r["rec_off1"] == -1).all() and (r["rec_off2"] == -1).all(), name
        assert set(r["rest1"] + r["rest2"] + r["guard1"] + r["guard2"]) <= {0xA5}, name
        return
    assert r["rc"] == 0 and r["n_records"] == c.n == st["records"], (name, r["rc"])
    assert r["out1"] == c.out1 and r["out2"] == c.out2, name
    assert r["guard1"] == r["guard2"] == b"\xa5" * 8 and set(r["rest1"] + r["rest2"]) <= {0xA5}, name      # nothing behind the prepared text
    assert r["rec_off1"][:c.n + 1].tolist() == c.off1.tolist() and (r["rec_off1"][c.n + 1:] == -1).all(), name
    assert r["rec_off2"][:c.n + 1].tolist() == c.off2.tolist() and (r["rec_off2"][c.n + 1:] == -1).all(), name
    assert (st["format"], st["decided_by"]) == (sc.NAMES[c.found], c.decided), name
    assert (st["skipped_lines"], st["runs"], st["distinct"], st["longest_barcode"]) == (c.skipped, c.runs, c.distinct, c.longest), (name, st)
    assert (st["with_barcode"], st["valid"]) == (c.with_bc, c.valid), name
    assert (st["bytes_in_r1"], st["bytes_in_r2"], st["bytes_out_r1"], st["bytes_out_r2"]) == (len(c.t1), len(c.t2), len(c.out1), len(c.out2)), name


# ---- 1. the kernels on texts in memory.  (r, w): the case's run size r (None: both texts in memory whole) at its window w, where that fits the run
SHAPES = [(r, w) for r in (None, 0, 1, 2) for w in range(3) if r is None or w <= r]


@pytest.mark.parametrize("slab", pc.SLABS)
@pytest.mark.parametrize("r,w", SHAPES)
def test_cases_through_the_kernels(r, w, slab):
    for name in pc.SMALL:
        c = pc.cases()[name]
        run_bytes = 0 if r is None else c.run_bytes[r]
        window = c.windows[w]
        res = api.selftest_fastq_prepare(c.t1, c.t2, c.format, run_bytes, window, slab)
        _hold(name, c, res)
        st = res["stats"]
        if c.exp is None:
            continue
        if slab == 1:
            assert st["slabs"] == c.n, name                              # one record a slab
        if slab == 4096 and "slabs" in c.claims:
            assert st["slabs"] > 1, name
        if w == 0 and r is None and "windows" in c.claims:
            assert st["windows"] > 1, name
        assert st["sorted_runs"] == 0 if r is None else st["sorted_runs"] >= (1 if c.n else 0), name
        if r is not None and "runs" in c.claims:
            assert st["sorted_runs"] >= len(c.t1) // run_bytes and st["tmp_bytes"] == len(c.out1) + len(c.out2), name


def test_a_few_thousand_records_at_the_defaults():
    c = pc.cases()["std_many"]
    res = api.selftest_fastq_prepare(c.t1, c.t2)
    print(res["stats"])
    _hold("many", c, res)
    assert res["stats"]["windows"] == 1 and res["stats"]["slabs"] == 1 and res["stats"]["sorted_runs"] == 0
    res = api.selftest_fastq_prepare(c.t1, c.t2, run_bytes=1 << 16)
    _hold("many in runs", c, res)
    assert res["stats"]["sorted_runs"] >= 4


def test_bad_arguments_small_room_and_a_record_longer_than_the_window_or_the_run():
    for window in (1, fc.MIN_WINDOW - 1, (1 << 29) + 1, -5):
        with pytest.raises(api.ArachneError) as e:
            api.selftest_fastq_prepare(b"", b"", "stlfr", 0, window)
        assert e.value.code == api.ARX_E_ARG
    for fmt in (4, 5, 9, -1):
        with pytest.raises(api.ArachneError) as e:
            api.selftest_fastq_prepare(b"", b"", fmt)
        assert e.value.code == api.ARX_E_ARG
    for run_bytes, window in ((fc.MIN_WINDOW - 1, 0), (255, 256), (-1, 0), (-7, fc.MIN_WINDOW)):
        with pytest.raises(api.ArachneError) as e:
            api.selftest_fastq_prepare(b"", b"", "stlfr", run_bytes, window)
        assert e.value.code == api.ARX_E_ARG
    t1, t2 = sc.rec(b"n" * 200 + b"#1_2_3", 5, 5)
    for fmt in ("auto", "stlfr"):
        for run_bytes, window in ((0, fc.MIN_WINDOW), (fc.MIN_WINDOW, 0), (4096, fc.MIN_WINDOW)):
            r = api.selftest_fastq_prepare(t1, t2, fmt, run_bytes, window)
            assert r["rc"] == api.ARX_E_TOO_LARGE and r["n_records"] == -1, (fmt, run_bytes)
            assert set(r["rest1"] + r["rest2"]) == {0xA5} and (r["rec_off1"] == -1).all() and (r["rec_off2"] == -1).all() and (r["out_len"] == -1).all()     # untouched
    c = pc.Case(t1 + sc.rec(b"a#0_2_3", 4, 4)[0], t2 + sc.rec(b"a#0_2_3", 4, 4)[1])
    assert c.out1 != c.std.out1
    for run_bytes in (0, 256):
        _hold("long", c, api.selftest_fastq_prepare(c.t1, c.t2, "auto", run_bytes, 256))
        r = api.selftest_fastq_prepare(c.t1, c.t2, "auto", run_bytes, 256, cap1=len(c.out1) - 1)      # an output that its room does not hold
        assert r["rc"] == api.ARX_E_TOO_LARGE and r["n_records"] == -1 and set(r["rest1"] + r["rest2"]) == {0xA5}
        r = api.selftest_fastq_prepare(c.t1, c.t2, "auto", run_bytes, 256, cap2=len(c.out2) - 1)
        assert r["rc"] == api.ARX_E_TOO_LARGE and r["n_records"] == -1 and set(r["rest1"] + r["rest2"]) == {0xA5}
        _hold("exact", c, api.selftest_fastq_prepare(c.t1, c.t2, "auto", run_bytes, 256, cap1=len(c.out1), cap2=len(c.out2)))
    s = pc.cases()["standard_auto"]                                          # the caps hold where the call is the sort itself
    r = api.selftest_fastq_prepare(s.t1, s.t2, cap1=len(s.out1) - 1)
    assert r["rc"] == api.ARX_E_TOO_LARGE and r["n_records"] == -1 and set(r["rest1"] + r["rest2"]) == {0xA5}


# ---- 2. and 3. files
RUN_FILES = 4096


@pytest.mark.parametrize("run_bytes", (0, RUN_FILES))
def test_files_of_every_form_equal_the_restatement_and_the_two_calls(tmp_path, run_bytes):
    c = pc.cases()["run_borders"]
    d = str(tmp_path)
    out, tmp, two = (os.path.join(d, x) for x in ("out", "tmp", "two"))
    for x in (out, tmp, two):
        os.mkdir(x)
    for form, (p1, p2) in _write_forms(d, c).items():
        for bgzf in (False, True):
            o1, o2 = (os.path.join(out, "out_%s_%d_%d.fq" % (form, bgzf, k)) for k in (1, 2))
            st = api.fastq_prepare(p1, p2, o1, o2, bgzf=bgzf, timed=bgzf, run_bytes=run_bytes, tmp_dir=tmp)
            print(form, bgzf, st)
            got1, got2 = _read_output(o1, bgzf), _read_output(o2, bgzf)
            assert got1 == c.out1 and got2 == c.out2, (form, bgzf)
            assert os.listdir(tmp) == [] and sorted(os.listdir(out)) == sorted(os.path.basename(o) for o in (o1, o2))
            assert (st["records"], st["skipped_lines"], st["format"], st["decided_by"], st["with_barcode"], st["valid"]) == (c.n, c.skipped, "stlfr", 0, c.with_bc, c.valid)
            assert (st["runs"], st["distinct"], st["longest_barcode"]) == (c.runs, c.distinct, c.longest)
            assert (st["bytes_in_r1"], st["bytes_in_r2"], st["bytes_out_r1"], st["bytes_out_r2"]) == (len(c.t1), len(c.t2), len(c.out1), len(c.out2))
            assert (st["sorted_runs"] >= 2 and st["tmp_bytes"] == len(c.out1) + len(c.out2)) if run_bytes else (st["sorted_runs"], st["tmp_bytes"]) == (0, 0)
            # the product's own two calls, which this work does not change, on the same files
            s1, s2, q1, q2 = (os.path.join(two, x) for x in ("std1.fq", "std2.fq", "srt1.fq", "srt2.fq"))
            api.fastq_standardize(p1, p2, s1, s2, bgzf=bgzf)
            ex = api.fastq_sort_ex(s1, s2, q1, q2, bgzf=bgzf, run_bytes=run_bytes, tmp_dir=tmp)
            assert _read_output(q1, bgzf) == got1 and _read_output(q2, bgzf) == got2, (form, bgzf)
            assert open(q1, "rb").read() == open(o1, "rb").read() and open(q2, "rb").read() == open(o2, "rb").read(), (form, bgzf)     # the files themselves
            for k in ("records", "runs", "distinct", "longest_barcode", "bytes_out_r1", "bytes_out_r2", "sort_passes", "slabs"):
                assert ex[k] == st[k], (form, bgzf, k)
            for o in (o1, o2):
                os.remove(o)


def test_the_two_calls_on_keys_in_two_pieces_and_on_empty_outputs(tmp_path):
    d = str(tmp_path)
    for name in ("key_in_id", "key_edges", "key_stlfr", "key_tell", "std_ids", "std_empty_forced"):
        c = pc.cases()[name]
        p1, p2 = devfeed.write(d, name + "_1.fq", c.t1), devfeed.write(d, name + "_2.fq", c.t2)
        o1, o2, s1, s2, q1, q2 = (os.path.join(d, name + x) for x in ("_o1.fq", "_o2.fq", "_s1.fq", "_s2.fq", "_q1.fq", "_q2.fq"))
        for run_bytes in (0, 256):
            for bgzf in (False, True):
                st = api.fastq_prepare(p1, p2, o1, o2, format=c.format, bgzf=bgzf, run_bytes=run_bytes)
                api.fastq_standardize(p1, p2, s1, s2, format=c.format)
                api.fastq_sort_ex(s1, s2, q1, q2, bgzf=bgzf, run_bytes=run_bytes)
                assert open(q1, "rb").read() == open(o1, "rb").read() and open(q2, "rb").read() == open(o2, "rb").read(), (name, run_bytes, bgzf)
                assert _read_output(o1, bgzf) == c.out1 and _read_output(o2, bgzf) == c.out2 and st["records"] == c.n, (name, run_bytes, bgzf)


# ---- 4. the property
@pytest.mark.parametrize("fmt", (sc.HAPLOTAGGING, sc.STLFR, sc.TELLSEQ))
def test_the_host_feeder_reads_every_barcode_of_the_output_as_one_set(tmp_path, fmt):
    raw = sc.Case(*sc.raw_pair(fmt, 90, seed=fmt))
    rng = np.random.default_rng(fmt)
    shuffled = [raw.recs[k] for k in rng.permutation(raw.n)]
    c = pc.Case(b"".join(r[0] for r in shuffled), b"".join(r[1] for r in shuffled))
    assert c.found == fmt and c.with_bc == c.n == 90 and 0 < c.valid < c.n and c.runs > c.distinct
    d = str(tmp_path)
    p1, p2 = devfeed.write(d, "raw1.fq", c.t1), devfeed.write(d, "raw2.fq", c.t2)
    o1, o2 = os.path.join(d, "prep1.fq"), os.path.join(d, "prep2.fq")
    st = api.fastq_prepare(p1, p2, o1, o2)
    assert st["format"] == sc.NAMES[fmt] and open(o1, "rb").read() == c.out1 and open(o2, "rb").read() == c.out2
    fd = api.Feeder(o1, o2)                                              # the host feeder is the yardstick
    batches = devfeed.feed_all(fd, 20)
    fd.close()
    got = _pairs_of(batches)
    assert len(got) == c.n and sum(b["n_sets"] for b in batches) == c.distinct == len({f[1] for f in c.std.fields})     # every barcode is one set
    order = sorted(range(c.n), key=lambda k: c.std.fields[k][1])
    code = lambda s: bytes(devfeed.nt4(chr(x)) for x in s)
    for g, k in zip(got, order):
        (r1, r2, _), (ident, bc, v) = c.std.recs[k], c.std.fields[k]
        l1, l2 = r1.split(b"\n"), r2.split(b"\n")
        assert g == (bc, bool(v), ident, code(l1[1]), l1[3], code(l2[1]), l2[3]), ident
    chk = api.fastq_sort(o1, o2, check=True)
    assert chk["runs"] == chk["distinct"] == c.distinct and chk["records"] == c.n


# ---- 5. CHECK, a standard pair, e2e.prepare
def test_check_a_standard_pair_and_e2e_prepare(tmp_path):
    d = str(tmp_path)
    out, tmp = os.path.join(d, "out"), os.path.join(d, "tmp")
    os.mkdir(out)
    os.mkdir(tmp)
    o1, o2 = os.path.join(out, "o1.fq"), os.path.join(out, "o2.fq")
    cs = pc.cases()
    paths = {n: tuple(devfeed.write(d, "%s_%d.fq" % (n, k), t) for k, t in ((1, cs[n].t1), (2, cs[n].t2))) for n in ("run_borders", "standard_auto", "std_det_plain")}
    c = cs["run_borders"]
    for run_bytes in (0, RUN_FILES):
        for outs in ((None, None), (o1, o2)):
            st = api.fastq_prepare(*paths["run_borders"], *outs, check=True, run_bytes=run_bytes, tmp_dir=tmp)      # nothing is written, whatever is passed
            assert os.listdir(out) == [] and os.listdir(tmp) == []
            assert (st["records"], st["runs"], st["distinct"], st["format"], st["with_barcode"], st["valid"]) == (c.n, c.runs, c.distinct, "stlfr", c.with_bc, c.valid)
            assert (st["bytes_out_r1"], st["bytes_out_r2"], st["slabs"], st["tmp_bytes"]) == (0, 0, 0, 0) and st["runs"] != st["distinct"]
    s = cs["standard_auto"]
    for run_bytes in (0, 128):
        st = api.fastq_prepare(*paths["standard_auto"], o1, o2, run_bytes=run_bytes)                         # "auto" on a standard pair: the sort itself
        assert (st["format"], st["decided_by"], st["records"], st["with_barcode"], st["valid"]) == ("standard", 0, s.n, 0, 0)
        assert open(o1, "rb").read() == s.out1 and open(o2, "rb").read() == s.out2 and s.out1 != s.t1
        ex = api.fastq_sort_ex(*paths["standard_auto"], os.path.join(d, "x1.fq"), os.path.join(d, "x2.fq"), run_bytes=run_bytes)
        assert open(os.path.join(d, "x1.fq"), "rb").read() == s.out1 and all(ex[k] == st[k] for k in ex if not k.endswith("_us"))
    # e2e.prepare: a standard pair that is sorted already is returned as it is; anything else is written
    g1, g2 = devfeed.write(d, "good_1.fq", s.out1), devfeed.write(d, "good_2.fq", s.out2)
    r1, r2, st = e2e.prepare(g1, g2, os.path.join(d, "e2e"))
    assert (r1, r2) == (g1, g2) and not st["prepared"] and st["format"] == "standard" and not os.path.exists(os.path.join(d, "e2e"))
    r1, r2, st = e2e.prepare(*paths["standard_auto"], os.path.join(d, "e2e"))
    assert st["prepared"] and r1.endswith("standard_auto_1.prepared.fastq") and open(r1, "rb").read() == s.out1 and open(r2, "rb").read() == s.out2
    r1, r2, st = e2e.prepare(*paths["run_borders"], os.path.join(d, "e2e"), bgzf=True, run_bytes=RUN_FILES, tmp_dir=tmp)
    assert st["prepared"] and st["format"] == "stlfr" and r1.endswith("run_borders_1.prepared.fastq.gz") and st["sorted_runs"] >= 2 and os.listdir(tmp) == []
    assert _read_output(r1, True) == c.out1 and _read_output(r2, True) == c.out2
    r1, r2, st = e2e.prepare(g1, g2, os.path.join(d, "e2e"), format="haplotagging", if_needed=False)      # a forced format converts even a good pair
    f = pc.Case(s.out1, s.out2, pc.HAPLOTAGGING)
    assert st["prepared"] and open(r1, "rb").read() == f.out1 and open(r2, "rb").read() == f.out2
    for kw in (dict(), dict(if_needed=False)):
        with pytest.raises(api.ArachneError) as e:
            e2e.prepare(*paths["std_det_plain"], os.path.join(d, "e2e_none"), **kw)
        assert e.value.code == api.ARX_E_ARG and e.value.stats["format"] == "unknown"


# ---- 6. what is refused
def test_what_is_refused_leaves_nothing_behind(tmp_path):
    d = str(tmp_path)
    c = pc.cases()["run_borders"]
    forms = _write_forms(d, c)
    p1, p2 = forms["bgzf"]
    out, tmp = os.path.join(d, "out"), os.path.join(d, "tmp")
    os.mkdir(out)
    os.mkdir(tmp)
    o1, o2 = os.path.join(out, "o1.fq"), os.path.join(out, "o2.fq")

    def refused(code, *a, **kw):
        kw.setdefault("tmp_dir", tmp)
        with pytest.raises(api.ArachneError) as e:
            api.fastq_prepare(*a, **kw)
        assert e.value.code == code, str(e.value)
        assert os.listdir(out) == [] and os.listdir(tmp) == []            # neither an output, a .tmp nor a run file
        return e.value

    u = pc.cases()["std_det_200"]
    u1, u2 = devfeed.write(d, "u1.fq", u.t1), devfeed.write(d, "u2.fq", u.t2)
    for rb in (0, RUN_FILES):
        e = refused(api.ARX_E_ARG, u1, u2, o1, o2, run_bytes=rb)           # unknown under "auto"
        assert "200" in str(e) and "format" in str(e) and e.stats["format"] == "unknown"
    for fmt in (4, 5, 9):
        refused(api.ARX_E_ARG, p1, p2, o1, o2, format=fmt)
    for rb in (-2, 1, fc.MIN_WINDOW - 1):
        refused(api.ARX_E_ARG, p1, p2, o1, o2, run_bytes=rb)
    raw = bytearray(open(p1, "rb").read())
    blocks = bgzfio.split(bytes(raw))
    assert len(blocks) > 1
    k = len(blocks) - 2                                                  # the last block with data: behind the first run's end
    raw[blocks[k]["at"] + blocks[k]["size"] - 8] ^= 0x55                 # a CRC that does not match: a status of the inflate kernel
    bad = os.path.join(d, "badcrc.fq.gz")
    with open(bad, "wb") as f:
        f.write(raw)
    for rb in (0, RUN_FILES):
        assert "inflate" in str(refused(api.ARX_E_IO, bad, p2, o1, o2, format="stlfr", run_bytes=rb))
        refused(api.ARX_E_IO, os.path.join(d, "no_such_file.fq"), p2, o1, o2, run_bytes=rb)
        refused(api.ARX_E_IO, p1, os.path.join(d, "no_such_file.fq"), check=True, run_bytes=rb)
        not_a_dir = os.path.join(d, "in_plain_1.fq", "o1.fq")           # under a regular file: unwritable whoever runs the test
        refused(api.ARX_E_IO, p1, p2, not_a_dir, o2, run_bytes=rb)
        refused(api.ARX_E_IO, p1, p2, o1, not_a_dir, run_bytes=rb)
        refused(api.ARX_E_TOO_LARGE, p1, p2, o1, o2, max_bytes=len(c.t1), run_bytes=rb)                    # more than max_bytes
    refused(api.ARX_E_IO, p1, p2, o1, o2, run_bytes=RUN_FILES, tmp_dir=os.path.join(d, "in_plain_1.fq"))  # a tmp_dir that is no directory
    long1, long2 = sc.rec(b"n" * 200 + b"#1_2_3", 5, 5)
    l1, l2 = devfeed.write(d, "long1.fq", c.t1 + long1), devfeed.write(d, "long2.fq", c.t2 + long2)
    e = refused(api.ARX_E_TOO_LARGE, l1, l2, o1, o2, run_bytes=fc.MIN_WINDOW)                             # a record that a run does not hold
    assert "run_bytes" in str(e)
    for a in forms["plain"]:
        refused(api.ARX_E_ARG, *forms["plain"], a, o2)                   # an output path that is an input
        refused(api.ARX_E_ARG, *forms["plain"], o1, os.path.join(d, ".", os.path.basename(a)))
    refused(api.ARX_E_ARG, p1, p2, o1, o1)
    refused(api.ARX_E_ARG, p1, p2, None, o2)
    lib = api._load(api.LIB_PATH)
    fn = api._selftest_fn(lib, "arx_fastq_prepare")
    msg_buf = C.create_string_buffer(256)
    for flags in (4, 0x200, 0x80):
        assert fn(0, p1.encode(), p2.encode(), o1.encode(), o2.encode(), 0, flags, 0, 0, None, None, msg_buf, 256) == api.ARX_E_ARG and b"flag" in msg_buf.value
    assert os.listdir(out) == [] and os.listdir(tmp) == []
    # the inputs are as they were, and the process prepares a good pair afterwards
    assert open(forms["plain"][0], "rb").read() == c.t1 and open(forms["plain"][1], "rb").read() == c.t2
    st = api.fastq_prepare(p1, p2, o1, o2, run_bytes=RUN_FILES, tmp_dir=tmp)
    assert st["records"] == c.n and open(o1, "rb").read() == c.out1 and open(o2, "rb").read() == c.out2
    assert sorted(os.listdir(out)) == ["o1.fq", "o2.fq"] and os.listdir(tmp) == []

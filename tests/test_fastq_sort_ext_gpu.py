"""The external sort of a FASTQ file pair on the GPU (arx_fastq_sort_ex, arx_selftest_fastq_sort_ext; arachne_amd/csrc/dev_fqmerge.h,
hip_fqsort.h): sorted runs, merged on the device.  1. the cases of fqsortcases.py and the run-border cases of fqextcases.py -- the ones
tests/test_fastq_sort_ext_sim.py runs through the host program -- through the kernels, held to the restatement, which knows of no runs;
2. files: plain, gzip and BGZF inputs through temporary run files into plain and BGZF outputs; 3. what is refused, and that neither outputs
nor temporary files are left behind; 4. the host feeder delivers from an externally sorted pair what it delivers from the unshuffled files."""
import ctypes as C
import os

import numpy as np
import pytest

import devfeed
import fqextcases as xc
import fqsortcases as fc
from arachne_amd import api, e2e
from test_fastq_sort_gpu import _hold, _read_output, _write_forms

pytestmark = pytest.mark.gpu


def _hold_ext(name, c, r, run_bytes):
    _hold(name, c, r)
    st = r["stats"]
    assert st["sorted_runs"] >= xc.least_runs(c, run_bytes), (name, run_bytes)
    assert st["tmp_bytes"] == len(c.out1) + len(c.out2), name             # the runs hold every record once


# ---- 1. the kernels on texts in memory
@pytest.mark.parametrize("slab", fc.SLABS)
@pytest.mark.parametrize("run_bytes", xc.RUN_BYTES)
def test_cases_through_the_kernels(run_bytes, slab):
    todo = [(n, fc.cases()[n]) for n in fc.SMALL] + [(n, xc.cases()[n].case) for n in xc.GOOD]
    for name, c in todo:
        r = api.selftest_fastq_sort_ext(c.t1, c.t2, run_bytes, fc.MIN_WINDOW, slab)
        print(name, run_bytes, slab, r["stats"])
        _hold_ext(name, c, r, run_bytes)
        if slab == 1:
            assert r["stats"]["slabs"] == c.n, name
        x = xc.cases().get(name)
        if x is not None and x.run_bytes == run_bytes:
            assert r["stats"]["sorted_runs"] >= x.min_runs, name
            if x.exact_runs is not None:
                assert r["stats"]["sorted_runs"] == x.exact_runs, name


def test_many_records_in_sixteen_runs_equal_the_in_core_sort():
    c = fc.cases()["many"]
    rb = 150000
    assert xc.least_runs(c, rb) >= 16
    r = api.selftest_fastq_sort_ext(c.t1, c.t2, rb)                      # window and slab at their defaults
    core = api.selftest_fastq_sort(c.t1, c.t2)
    print(r["stats"])
    assert r["stats"]["sorted_runs"] >= 16
    assert r["out1"] == core["out1"] and r["out2"] == core["out2"] and r["n_records"] == core["n_records"]
    assert (r["rec_off1"] == core["rec_off1"]).all() and (r["rec_off2"] == core["rec_off2"]).all()
    for k in ("records", "skipped_lines", "runs", "distinct", "longest_barcode", "sort_passes", "slabs", "bytes_out_r1", "bytes_out_r2"):
        assert r["stats"][k] == core["stats"][k], k
    _hold_ext("many", c, r, rb)


def test_what_the_self_test_refuses():
    for name in xc.REFUSED:
        x = xc.cases()[name]
        r = api.selftest_fastq_sort_ext(x.case.t1, x.case.t2, x.run_bytes, fc.MIN_WINDOW, 4096)
        assert r["rc"] == api.ARX_E_TOO_LARGE and r["n_records"] == -1, name
        assert set(r["out1"] + r["out2"]) == {0xA5} and (r["rec_off1"] == -1).all() and (r["rec_off2"] == -1).all(), name   # untouched
    for run_bytes, window in ((fc.MIN_WINDOW - 1, fc.MIN_WINDOW), (255, 256), (0, fc.MIN_WINDOW), (-1, fc.MIN_WINDOW)):
        with pytest.raises(api.ArachneError) as e:
            api.selftest_fastq_sort_ext(b"", b"", run_bytes, window)
        assert e.value.code == api.ARX_E_ARG


# ---- 2. files
def test_files_of_every_form_through_run_files(tmp_path):
    c = fc.cases()["three_hundred"]
    d = str(tmp_path)
    forms = _write_forms(d, c)
    tmp, out = os.path.join(d, "tmp"), os.path.join(d, "out")
    os.mkdir(tmp)
    os.mkdir(out)
    rb = 4096
    assert xc.least_runs(c, rb) >= 5
    for form, (p1, p2) in forms.items():
        chk = api.fastq_sort_ex(p1, p2, check=True, run_bytes=rb)         # no tmp_dir, no output directory: nothing is written
        core = api.fastq_sort(p1, p2, check=True)
        for k in ("records", "skipped_lines", "runs", "distinct", "longest_barcode", "bytes_in_r1", "bytes_in_r2", "bytes_out_r1", "bytes_out_r2", "slabs"):
            assert chk[k] == core[k], (form, k)
        assert chk["sorted_runs"] >= 5 and chk["tmp_bytes"] == 0
        for bgzf in (False, True):
            o1, o2 = (os.path.join(out, "out_%s_%d_%d.fq" % (form, bgzf, k)) for k in (1, 2))
            st = api.fastq_sort_ex(p1, p2, o1, o2, bgzf=bgzf, timed=bgzf, run_bytes=rb, tmp_dir=tmp)
            print(form, bgzf, st)
            assert _read_output(o1, bgzf) == c.out1 and _read_output(o2, bgzf) == c.out2, (form, bgzf)
            assert os.listdir(tmp) == [] and sorted(os.listdir(out)) == sorted(os.path.basename(o) for o in (o1, o2))
            assert (st["records"], st["skipped_lines"], st["runs"], st["distinct"]) == (c.n, 0, c.runs, c.distinct)
            assert (st["bytes_in_r1"], st["bytes_in_r2"], st["bytes_out_r1"], st["bytes_out_r2"]) == (len(c.t1), len(c.t2), len(c.out1), len(c.out2))
            assert st["sorted_runs"] >= 5 and st["tmp_bytes"] == len(c.out1) + len(c.out2)
            os.remove(o1)
            os.remove(o2)
    p1, p2 = forms["bgzf"]
    o1, o2 = os.path.join(out, "a.fq"), os.path.join(out, "b.fq")
    st = api.fastq_sort_ex(p1, p2, o1, o2, run_bytes=rb)                  # tmp_dir None: the directory of r1_out
    assert open(o1, "rb").read() == c.out1 and sorted(os.listdir(out)) == ["a.fq", "b.fq"]
    same = api.fastq_sort_ex(p1, p2, o1, o2, run_bytes=0, tmp_dir=os.path.join(d, "in_plain_1.fq", "x"))      # exactly arx_fastq_sort: tmp_dir is ignored
    core = api.fastq_sort(p1, p2, o1, o2)
    counts = [k for k in core if not k.endswith("_us")]
    assert [same[k] for k in counts] == [core[k] for k in counts] and set(same) - set(core) == {"sorted_runs", "tmp_bytes", "run_write_us", "run_read_us"}
    assert same["sorted_runs"] == same["tmp_bytes"] == same["run_write_us"] == same["run_read_us"] == 0
    auto = api.fastq_sort_ex(p1, p2, check=True, run_bytes=-1)            # the library's own run size holds this pair in one run
    assert auto["sorted_runs"] == 1 and auto["records"] == c.n


def test_presort_passes_run_bytes_on(tmp_path):
    d = str(tmp_path)
    cs = fc.cases()
    paths = {name: tuple(devfeed.write(d, "%s_%d.fq" % (name, k), t) for k, t in ((1, cs[name].t1), (2, cs[name].t2))) for name in ("sorted_clean", "three_hundred")}
    r1, r2, st = e2e.presort(*paths["sorted_clean"], os.path.join(d, "out"), run_bytes=128)
    assert (r1, r2) == paths["sorted_clean"] and not st["sorted"] and st["sorted_runs"] > 1 and not os.path.exists(os.path.join(d, "out"))
    tmp = os.path.join(d, "tmp")
    os.mkdir(tmp)
    r1, r2, st = e2e.presort(*paths["three_hundred"], os.path.join(d, "out"), run_bytes=4096, tmp_dir=tmp)
    assert st["sorted"] and st["sorted_runs"] >= 5 and open(r1, "rb").read() == cs["three_hundred"].out1 and open(r2, "rb").read() == cs["three_hundred"].out2
    assert os.listdir(tmp) == []


# ---- 3. what is refused
def test_what_is_refused_leaves_nothing_behind(tmp_path):
    import bgzfio
    d = str(tmp_path)
    c = fc.cases()["three_hundred"]
    forms = _write_forms(d, c)
    p1, p2 = forms["bgzf"]
    out, tmp = os.path.join(d, "out"), os.path.join(d, "tmp")
    os.mkdir(out)
    os.mkdir(tmp)
    o1, o2 = os.path.join(out, "o1.fq"), os.path.join(out, "o2.fq")
    rb = 4096

    def refused(code, *a, **kw):
        with pytest.raises(api.ArachneError) as e:
            api.fastq_sort_ex(*a, **dict(dict(run_bytes=rb, tmp_dir=tmp), **kw))
        assert e.value.code == code, str(e.value)
        assert os.listdir(out) == [] and os.listdir(tmp) == []           # neither an output, a .tmp nor a run file
        return str(e.value)

    raw = bytearray(open(p1, "rb").read())
    blocks = bgzfio.split(bytes(raw))
    assert len(blocks) > 3 and sum(b["isize"] for b in blocks[:2]) > rb  # the damaged block lies behind the first run's end
    raw[blocks[2]["at"] + blocks[2]["size"] - 8] ^= 0x55
    bad = os.path.join(d, "badcrc.fq.gz")
    with open(bad, "wb") as f:
        f.write(raw)
    assert "inflate" in refused(api.ARX_E_IO, bad, p2, o1, o2)
    refused(api.ARX_E_IO, bad, p2, check=True)
    refused(api.ARX_E_IO, p1, p2, o1, o2, tmp_dir=os.path.join(d, "in_plain_1.fq", "t"))      # under a regular file: unwritable whoever runs the test
    refused(api.ARX_E_IO, p1, p2, os.path.join(d, "in_plain_1.fq", "o1.fq"), o2)
    refused(api.ARX_E_TOO_LARGE, p1, p2, o1, o2, max_bytes=len(c.t1) + len(c.t2) - 1)
    assert api.fastq_sort_ex(p1, p2, check=True, run_bytes=rb, max_bytes=len(c.t1) + len(c.t2))["records"] == c.n
    refused(api.ARX_E_ARG, p1, p2, o1, o2, run_bytes=fc.MIN_WINDOW - 1)
    refused(api.ARX_E_ARG, p1, p2, o1, o2, run_bytes=-2)
    refused(api.ARX_E_ARG, p1, p2, o1, o1)
    refused(api.ARX_E_ARG, p1, p2, None, o2)
    refused(api.ARX_E_ARG, *forms["plain"], forms["plain"][0], o2)
    x = xc.cases()["too_long"]
    q1, q2 = devfeed.write(d, "long1.fq", x.case.t1), devfeed.write(d, "long2.fq", x.case.t2)
    assert "larger run_bytes" in refused(api.ARX_E_TOO_LARGE, q1, q2, o1, o2, run_bytes=x.run_bytes)
    x = xc.cases()["over_cap"]
    q1, q2 = devfeed.write(d, "cap1.fq", x.case.t1), devfeed.write(d, "cap2.fq", x.case.t2)
    assert "larger run_bytes" in refused(api.ARX_E_TOO_LARGE, q1, q2, o1, o2, run_bytes=x.run_bytes)
    fn = api._selftest_fn(api._load(api.LIB_PATH), "arx_fastq_sort_ex")
    msg_buf = C.create_string_buffer(256)
    assert fn(0, p1.encode(), p2.encode(), o1.encode(), o2.encode(), 4, 0, rb, tmp.encode(), None, msg_buf, 256) == api.ARX_E_ARG and b"flag" in msg_buf.value
    assert os.listdir(out) == [] and os.listdir(tmp) == []
    # the inputs are as they were, and the process sorts a good file afterwards
    assert open(forms["plain"][0], "rb").read() == c.t1 and open(forms["plain"][1], "rb").read() == c.t2
    st = api.fastq_sort_ex(p1, p2, o1, o2, run_bytes=rb, tmp_dir=tmp)
    assert st["records"] == c.n and open(o1, "rb").read() == c.out1 and open(o2, "rb").read() == c.out2
    assert sorted(os.listdir(out)) == ["o1.fq", "o2.fq"] and os.listdir(tmp) == []


# ---- 4. the property that matters
def test_the_host_feeder_delivers_the_unshuffled_files(tmp_path):
    groups = [("A-1", 7), ("A-10", 2), ("B-7", 3), ("B-7-2", 6), ("CC", 1), ("D-1-2", 12), ("D-1-3", 5), ("a-1", 9)]
    bcs = [g[0].encode() for g in groups]
    t1, t2 = (t.encode() for t in devfeed.fastq(groups, seed=4))
    recs, skipped = fc.records(t1, t2)
    assert skipped == 0 and [r[2] for r in recs] == [b for b, g in zip(bcs, groups) for _ in range(g[1])]
    rng = np.random.default_rng(12)                                      # a seeded shuffle that keeps the order inside every barcode
    order = [recs[k][2] for k in rng.permutation(len(recs))]
    queues = {b: [r for r in recs if r[2] == b] for b in bcs}
    shuffled = [queues[b].pop(0) for b in order]
    assert shuffled != recs and sorted(shuffled, key=lambda r: r[2]) == recs
    d = str(tmp_path)
    p1, p2 = devfeed.write(d, "shuf1.fq", b"".join(r[0] for r in shuffled)), devfeed.write(d, "shuf2.fq", b"".join(r[1] for r in shuffled))
    o1, o2 = os.path.join(d, "sorted1.fq"), os.path.join(d, "sorted2.fq")
    rb = max(fc.MIN_WINDOW, 2 * max(max(len(r[0]), len(r[1])) for r in recs))
    st = api.fastq_sort_ex(p1, p2, o1, o2, run_bytes=rb)
    assert st["runs"] > st["distinct"] == len(groups) and st["sorted_runs"] >= 4
    u1, u2 = devfeed.write(d, "orig1.fq", t1), devfeed.write(d, "orig2.fq", t2)
    batches = {}
    for tag, (a, b) in (("sorted", (o1, o2)), ("original", (u1, u2))):
        fd = api.Feeder(a, b)                                            # the host feeder is the yardstick
        batches[tag] = devfeed.feed_all(fd, 20)
        fd.close()
    devfeed.assert_same_batches(batches["sorted"], batches["original"])
    assert sum(b["n_sets"] for b in batches["sorted"]) == len(groups)    # every barcode is one set
    assert open(o1, "rb").read() == t1 and open(o2, "rb").read() == t2

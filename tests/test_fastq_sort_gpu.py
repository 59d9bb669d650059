"""The sort of a FASTQ file pair by barcode on the GPU (arx_fastq_sort, arx_selftest_fastq_sort; arachne_amd/csrc/dev_fqsort.h, hip_fqsort.h).
1. the cases of fqsortcases.py -- the ones tests/test_fastq_sort_sim.py runs through the host program -- through the kernels, held to the
restatement there; 2. files: plain, gzip and BGZF inputs into plain and BGZF outputs; 3. the property the sort exists for: the host feeder
delivers from the sorted pair what it delivers from the files before they were shuffled; 4. what is refused, and that nothing is left behind."""
import gzip
import os

import numpy as np
import pytest

import bgzfio
import devfeed
import fqsortcases as fc
from arachne_amd import api, e2e, synth

pytestmark = pytest.mark.gpu


def _hold(name, c, r):
    st = r["stats"]
    assert r["rc"] == 0 and r["n_records"] == c.n == st["records"], name
    assert r["out1"] == c.out1 and r["out2"] == c.out2, name
    assert r["guard1"] == r["guard2"] == b"\xa5" * 8 and set(r["rest1"] + r["rest2"]) <= {0xA5}, name      # nothing behind the sorted text
    assert r["rec_off1"][:c.n + 1].tolist() == c.off1.tolist() and (r["rec_off1"][c.n + 1:] == -1).all(), name
    assert r["rec_off2"][:c.n + 1].tolist() == c.off2.tolist() and (r["rec_off2"][c.n + 1:] == -1).all(), name
    assert (st["skipped_lines"], st["runs"], st["distinct"], st["longest_barcode"]) == (c.skipped, c.runs, c.distinct, c.longest), name
    assert (st["bytes_in_r1"], st["bytes_in_r2"], st["bytes_out_r1"], st["bytes_out_r2"]) == (len(c.t1), len(c.t2), len(c.out1), len(c.out2)), name


# ---- 1. the kernels on texts in memory
@pytest.mark.parametrize("slab", fc.SLABS)
@pytest.mark.parametrize("window", fc.WINDOWS)
def test_cases_through_the_kernels(window, slab):
    for name in fc.SMALL:
        c = fc.cases()[name]
        r = api.selftest_fastq_sort(c.t1, c.t2, window, slab)
        print(name, window, slab, r["stats"])
        _hold(name, c, r)
        st = r["stats"]
        if slab == 1:
            assert st["slabs"] == c.n, name                              # one record a slab
        if window == fc.MIN_WINDOW and "windows" in c.claims:
            assert st["windows"] > 1, name
        if slab == 4096 and "slabs" in c.claims:
            assert st["slabs"] > 1, name


def test_many_records_at_the_defaults():
    c = fc.cases()["many"]
    r = api.selftest_fastq_sort(c.t1, c.t2)
    print(r["stats"])
    _hold("many", c, r)
    assert r["stats"]["windows"] == 1 and r["stats"]["slabs"] == 1 and r["stats"]["sort_passes"] >= 3


def test_bad_arguments_and_a_record_longer_than_the_window():
    for window in (1, fc.MIN_WINDOW - 1, (1 << 29) + 1, -5):
        with pytest.raises(api.ArachneError) as e:
            api.selftest_fastq_sort(b"", b"", window)
        assert e.value.code == api.ARX_E_ARG
    t1, t2 = fc.pair(b"n" * 200, b"A-1", 5, 5)
    r = api.selftest_fastq_sort(t1, t2, fc.MIN_WINDOW)
    assert r["rc"] == api.ARX_E_TOO_LARGE and r["n_records"] == -1
    assert set(r["out1"] + r["out2"]) == {0xA5} and (r["rec_off1"] == -1).all() and (r["rec_off2"] == -1).all()     # untouched
    c = fc.Case(t1, t2)
    _hold("long", c, api.selftest_fastq_sort(t1, t2, 256))


# ---- 2. files
def _write_forms(d, c):
    """the case's two texts as plain, gzip and BGZF files -> {form: (r1, r2)}"""
    forms = {}
    for form in ("plain", "gzip", "bgzf"):
        ps = []
        for k, t in enumerate((c.t1, c.t2)):
            p = os.path.join(d, "in_%s_%d.fq" % (form, k + 1) + ("" if form == "plain" else ".gz"))
            with open(p, "wb") as f:
                f.write(t if form == "plain" else gzip.compress(t) if form == "gzip" else bgzfio.write_bgzf(t, cut=7001))
            ps.append(p)
        forms[form] = tuple(ps)
    return forms


def _read_output(p, bgzf):
    raw = open(p, "rb").read()
    if not bgzf:
        return raw
    assert raw.endswith(bgzfio.EOF_BLOCK)
    blocks = bgzfio.split(raw)
    assert blocks[-1]["isize"] == 0 and all(b["isize"] == bgzfio.BLOCK_IN for b in blocks[:-2]) and 0 < blocks[-2]["isize"] <= bgzfio.BLOCK_IN
    return bgzfio.inflate(raw)


def test_files_of_every_form(tmp_path):
    c = fc.cases()["three_hundred"]
    d = str(tmp_path)
    forms = _write_forms(d, c)
    for form, (p1, p2) in forms.items():
        chk = api.fastq_sort(p1, p2, check=True)
        assert chk["runs"] != chk["distinct"] and (chk["records"], chk["runs"], chk["distinct"]) == (c.n, c.runs, c.distinct), form
        assert chk["bytes_out_r1"] == chk["bytes_out_r2"] == chk["slabs"] == 0
        for bgzf in (False, True):
            o1, o2 = (os.path.join(d, "out_%s_%d_%d.fq" % (form, bgzf, k)) for k in (1, 2))
            st = api.fastq_sort(p1, p2, o1, o2, bgzf=bgzf, timed=bgzf)
            print(form, bgzf, st)
            assert _read_output(o1, bgzf) == c.out1 and _read_output(o2, bgzf) == c.out2, (form, bgzf)
            assert not os.path.exists(o1 + ".tmp") and not os.path.exists(o2 + ".tmp")
            assert (st["records"], st["skipped_lines"], st["runs"], st["distinct"]) == (c.n, 0, c.runs, c.distinct)
            assert (st["bytes_in_r1"], st["bytes_in_r2"], st["bytes_out_r1"], st["bytes_out_r2"]) == (len(c.t1), len(c.t2), len(c.out1), len(c.out2))
            again = api.fastq_sort(o1, o2, check=True)                   # the output, plain or BGZF, is sorted
            assert again["runs"] == again["distinct"] == c.distinct and again["records"] == c.n, (form, bgzf)


def test_a_bgzf_output_of_several_blocks(tmp_path):
    c = fc.cases()["many"]
    d = str(tmp_path)
    p1, p2 = os.path.join(d, "m1.fq.gz"), os.path.join(d, "m2.fq.gz")
    bgzfio.write_bgzf_file(p1, c.t1, level=1)
    with open(p2, "wb") as f:
        f.write(c.t2)                                                    # R1 BGZF, R2 plain: each file is judged by itself
    o1, o2 = os.path.join(d, "s1.fq.gz"), os.path.join(d, "s2.fq.gz")
    st = api.fastq_sort(p1, p2, o1, o2, bgzf=True)
    print(st)
    assert len(bgzfio.split(open(o1, "rb").read())) > 40
    assert _read_output(o1, True) == c.out1 and _read_output(o2, True) == c.out2


def test_presort_sorts_only_what_needs_it(tmp_path):
    d = str(tmp_path)
    cs = fc.cases()
    paths = {}
    for name in ("sorted_clean", "stability"):
        paths[name] = tuple(devfeed.write(d, "%s_%d.fq" % (name, k), t) for k, t in ((1, cs[name].t1), (2, cs[name].t2)))
    r1, r2, st = e2e.presort(*paths["sorted_clean"], os.path.join(d, "out"))
    assert (r1, r2) == paths["sorted_clean"] and not st["sorted"] and not os.path.exists(os.path.join(d, "out"))
    r1, r2, st = e2e.presort(*paths["stability"], os.path.join(d, "out"), bgzf=True)
    assert st["sorted"] and r1 != r2 and _read_output(r1, True) == cs["stability"].out1 and _read_output(r2, True) == cs["stability"].out2
    r1, r2, st = e2e.presort(*paths["sorted_clean"], os.path.join(d, "out2"), if_needed=False)
    assert st["sorted"] and open(r1, "rb").read() == cs["sorted_clean"].t1 and open(r2, "rb").read() == cs["sorted_clean"].t2


def test_the_device_feeder_reads_a_bgzf_output(tmp_path):
    d = str(tmp_path)
    c = fc.cases()["three_hundred"]
    p1, p2 = devfeed.write(d, "a1.fq", c.t1), devfeed.write(d, "a2.fq", c.t2)
    o1, o2 = os.path.join(d, "s1.fq.gz"), os.path.join(d, "s2.fq.gz")
    api.fastq_sort(p1, p2, o1, o2, bgzf=True)
    fa = os.path.join(d, "g.fa")
    synth.make_genome(3, [20000, 6000]).write_fasta(fa)
    api.index_build(fa, fa)
    ref = api.Reference(fa)
    try:
        fd = api.Feeder(o1, o2, device=ref, inflate="device")
        got = devfeed.feed_all(fd, 1000)
        st = fd.stats()
        fd.close()
    finally:
        ref.close()
    assert st["device_blocks"] > 0                                                  # its blocks were inflated on the device: it was taken for BGZF
    q1, q2 = devfeed.write(d, "plain1.fq", c.out1), devfeed.write(d, "plain2.fq", c.out2)
    fh = api.Feeder(q1, q2)
    want = devfeed.feed_all(fh, 1000)
    fh.close()
    devfeed.assert_same_batches(got, want)
    assert sum(b["n_sets"] for b in got) == c.distinct                   # every barcode is one set


# ---- 3. the property that matters: after the sort the feeder sees every barcode as one run, and the records are the input's
def test_the_host_feeder_delivers_the_unshuffled_files(tmp_path):
    groups = [("A-1", 7), ("A-10", 2), ("B-7", 3), ("B-7-2", 6), ("CC", 1), ("D-1-2", 12), ("D-1-3", 5), ("a-1", 9)]
    bcs = [g[0].encode() for g in groups]
    assert bcs == sorted(bcs) and len(set(bcs)) == len(bcs)              # ascending byte-wise
    t1, t2 = (t.encode() for t in devfeed.fastq(groups, seed=4))
    recs, skipped = fc.records(t1, t2)
    assert skipped == 0 and len(recs) == sum(g[1] for g in groups) and [r[2] for r in recs] == [b for b, g in zip(bcs, groups) for _ in range(g[1])]
    # a seeded shuffle of the records that keeps the order inside every barcode
    rng = np.random.default_rng(12)
    order = [recs[k][2] for k in rng.permutation(len(recs))]
    queues = {b: [r for r in recs if r[2] == b] for b in bcs}
    shuffled = [queues[b].pop(0) for b in order]
    assert shuffled != recs and sorted(shuffled, key=lambda r: r[2]) == recs
    d = str(tmp_path)
    p1, p2 = devfeed.write(d, "shuf1.fq", b"".join(r[0] for r in shuffled)), devfeed.write(d, "shuf2.fq", b"".join(r[1] for r in shuffled))
    o1, o2 = os.path.join(d, "sorted1.fq"), os.path.join(d, "sorted2.fq")
    st = api.fastq_sort(p1, p2, o1, o2)
    assert st["runs"] > st["distinct"] == len(groups)
    u1, u2 = devfeed.write(d, "orig1.fq", t1), devfeed.write(d, "orig2.fq", t2)
    batches = {}
    for tag, (a, b) in (("sorted", (o1, o2)), ("original", (u1, u2)), ("shuffled", (p1, p2))):
        fd = api.Feeder(a, b)                                            # the host feeder is the yardstick
        batches[tag] = devfeed.feed_all(fd, 20)
        fd.close()
    devfeed.assert_same_batches(batches["sorted"], batches["original"])
    assert sum(b["n_sets"] for b in batches["original"]) == len(groups) < sum(b["n_sets"] for b in batches["shuffled"])
    assert open(o1, "rb").read() == t1 and open(o2, "rb").read() == t2


# ---- 4. what is refused
def test_what_is_refused_leaves_nothing_behind(tmp_path):
    d = str(tmp_path)
    c = fc.cases()["three_hundred"]
    forms = _write_forms(d, c)
    p1, p2 = forms["bgzf"]
    out = os.path.join(d, "out")
    os.mkdir(out)
    o1, o2 = os.path.join(out, "o1.fq"), os.path.join(out, "o2.fq")

    def refused(code, *a, **kw):
        with pytest.raises(api.ArachneError) as e:
            api.fastq_sort(*a, **kw)
        assert e.value.code == code, str(e.value)
        assert os.listdir(out) == []                                     # neither an output nor a .tmp
        return str(e.value)

    raw = bytearray(open(p1, "rb").read())
    blocks = bgzfio.split(bytes(raw))
    assert len(blocks) > 3
    raw[blocks[2]["at"] + blocks[2]["size"] - 8] ^= 0x55                 # a CRC that does not match: a status of the inflate kernel
    bad = os.path.join(d, "badcrc.fq.gz")
    with open(bad, "wb") as f:
        f.write(raw)
    assert "inflate" in refused(api.ARX_E_IO, bad, p2, o1, o2)
    refused(api.ARX_E_IO, bad, p2, check=True)
    refused(api.ARX_E_IO, os.path.join(d, "no_such_file.fq"), p2, o1, o2)
    not_a_dir = os.path.join(d, "in_plain_1.fq", "o1.fq")               # under a regular file: unwritable whoever runs the test
    refused(api.ARX_E_IO, p1, p2, not_a_dir, o2)
    refused(api.ARX_E_IO, p1, p2, o1, not_a_dir)
    if os.geteuid() != 0:
        locked = os.path.join(d, "locked")
        os.mkdir(locked, 0o500)
        refused(api.ARX_E_IO, p1, p2, os.path.join(locked, "o1.fq"), o2)
        assert os.listdir(locked) == []
    msg = refused(api.ARX_E_TOO_LARGE, p1, p2, o1, o2, max_bytes=len(c.t1) + len(c.t2) - 1)
    assert "split the input" in msg and "per lane" in msg
    assert api.fastq_sort(p1, p2, check=True, max_bytes=len(c.t1) + len(c.t2))["records"] == c.n
    for a in forms["plain"]:
        refused(api.ARX_E_ARG, *forms["plain"], a, o2)                   # an output path that is an input
        refused(api.ARX_E_ARG, *forms["plain"], o1, os.path.join(d, ".", os.path.basename(a)))
    refused(api.ARX_E_ARG, p1, p2, o1, o1)
    refused(api.ARX_E_ARG, p1, p2, None, o2)
    lib = api._load(api.LIB_PATH)
    fn = api._selftest_fn(lib, "arx_fastq_sort")
    import ctypes as C
    msg_buf = C.create_string_buffer(256)
    assert fn(0, p1.encode(), p2.encode(), o1.encode(), o2.encode(), 4, 0, None, msg_buf, 256) == api.ARX_E_ARG and b"flag" in msg_buf.value
    assert os.listdir(out) == []
    # the inputs are as they were, and the process sorts a good file afterwards
    assert open(forms["plain"][0], "rb").read() == c.t1 and open(forms["plain"][1], "rb").read() == c.t2
    st = api.fastq_sort(p1, p2, o1, o2)
    assert st["records"] == c.n and open(o1, "rb").read() == c.out1 and open(o2, "rb").read() == c.out2
    assert sorted(os.listdir(out)) == ["o1.fq", "o2.fq"]

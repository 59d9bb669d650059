"""The header standardization of a FASTQ file pair on the GPU (arx_fastq_standardize, arx_selftest_fastq_standardize; arachne_amd/csrc/dev_fqstd.h,
hip_fqstd.h).  1. the cases of fqstdcases.py -- the ones tests/test_fastq_standardize_sim.py runs through the host program -- through the
kernels, held to the restatement there; 2. files: plain, gzip and BGZF inputs into plain and BGZF outputs; 3. the property the step exists
for: the host feeder reads from the output the restatement's barcode, validity and id and the input's bases and qualities, and the sort of the
output has every barcode in one run; 4. detection alone, and a pair that is standard already; 5. what is refused, and that nothing is left behind."""
import gzip
import os

import numpy as np
import pytest

import bgzfio
import devfeed
import fqstdcases as sc
from arachne_amd import api, e2e

pytestmark = pytest.mark.gpu


def _hold(name, c, r):
    st = r["stats"]
    if c.used is None:                                                       # "auto" found standard or unknown: nothing is written
        assert r["rc"] == (api.ARX_OK if c.found == sc.STANDARD else api.ARX_E_ARG), name
        assert (st["format"], st["decided_by"]) == (sc.NAMES[c.found], c.decided), name
        assert r["n_records"] == -1 and (r["out_len"] == -1).all() and (r["rec_off1"] == -1).all() and (r["rec_off2"] == -1).all(), name
        assert set(r["rest1"] + r["rest2"] + r["guard1"] + r["guard2"]) <= {0xA5}, name
        return
    assert r["rc"] == 0 and r["n_records"] == c.n == st["records"], name
    assert r["out1"] == c.out1 and r["out2"] == c.out2, name
    assert r["guard1"] == r["guard2"] == b"\xa5" * 8 and set(r["rest1"] + r["rest2"]) <= {0xA5}, name      # nothing behind the rewritten text
    assert r["rec_off1"][:c.n + 1].tolist() == c.off1.tolist() and (r["rec_off1"][c.n + 1:] == -1).all(), name
    assert r["rec_off2"][:c.n + 1].tolist() == c.off2.tolist() and (r["rec_off2"][c.n + 1:] == -1).all(), name
    assert st["format"] == sc.NAMES[c.used] and st["decided_by"] == (c.decided if c.format == sc.AUTO else -1), name
    assert (st["skipped_lines"], st["with_barcode"], st["valid"], st["longest_barcode"]) == (c.skipped, c.with_bc, c.valid, c.longest), name
    assert (st["bytes_out_r1"], st["bytes_out_r2"]) == (len(c.out1), len(c.out2)), name


# ---- 1. the kernels on texts in memory
@pytest.mark.parametrize("slab", sc.SLABS)
@pytest.mark.parametrize("w", range(3))
def test_cases_through_the_kernels(w, slab):
    for name in sc.SMALL:
        c = sc.cases()[name]
        window = c.windows[w]
        r = api.selftest_fastq_standardize(c.t1, c.t2, c.format, window, slab)
        print(name, window, slab, r["stats"])
        _hold(name, c, r)
        st = r["stats"]
        if c.used is None:
            continue
        if slab == 1:
            assert st["slabs"] == c.n, name                              # one record a slab
        if w == 0 and "windows" in c.claims:
            assert st["windows"] > 1, name
        if slab == 4096 and "slabs" in c.claims:
            assert st["slabs"] > 1, name


def test_many_records_at_the_defaults():
    c = sc.cases()["many"]
    r = api.selftest_fastq_standardize(c.t1, c.t2)
    print(r["stats"])
    _hold("many", c, r)
    assert r["stats"]["windows"] == 1 and r["stats"]["slabs"] == 1
    assert (r["stats"]["bytes_in_r1"], r["stats"]["bytes_in_r2"]) == (len(c.t1), len(c.t2))


def test_bad_arguments_small_room_and_a_record_longer_than_the_window():
    for window in (1, sc.MIN_WINDOW - 1, (1 << 29) + 1, -5):
        with pytest.raises(api.ArachneError) as e:
            api.selftest_fastq_standardize(b"", b"", "stlfr", window)
        assert e.value.code == api.ARX_E_ARG
    for fmt in (4, 5, 9, -1):
        with pytest.raises(api.ArachneError) as e:
            api.selftest_fastq_standardize(b"", b"", fmt)
        assert e.value.code == api.ARX_E_ARG
    t1, t2 = sc.rec(b"n" * 200 + b"#1_2_3", 5, 5)
    for fmt in ("auto", "stlfr"):
        r = api.selftest_fastq_standardize(t1, t2, fmt, sc.MIN_WINDOW)
        assert r["rc"] == api.ARX_E_TOO_LARGE and r["n_records"] == -1
        assert set(r["rest1"] + r["rest2"]) == {0xA5} and (r["rec_off1"] == -1).all() and (r["rec_off2"] == -1).all()     # untouched
    c = sc.Case(t1, t2)
    _hold("long", c, api.selftest_fastq_standardize(t1, t2, "auto", 256))
    r = api.selftest_fastq_standardize(t1, t2, "auto", 256, cap1=len(c.out1) - 1)          # an output that its room does not hold
    assert r["rc"] == api.ARX_E_TOO_LARGE and r["n_records"] == -1 and set(r["rest1"] + r["rest2"]) == {0xA5}
    _hold("exact", c, api.selftest_fastq_standardize(t1, t2, "auto", 256, cap1=len(c.out1), cap2=len(c.out2)))


# ---- 2. files
def _write_forms(d, c):
    """the case's two texts as plain, gzip and BGZF files -> {form: (r1, r2)}; "mixed": R1 BGZF, R2 gzip -- each file is judged by itself"""
    forms = {}
    for form in ("plain", "gzip", "bgzf"):
        ps = []
        for k, t in enumerate((c.t1, c.t2)):
            p = os.path.join(d, "in_%s_%d.fq" % (form, k + 1) + ("" if form == "plain" else ".gz"))
            with open(p, "wb") as f:
                f.write(t if form == "plain" else gzip.compress(t) if form == "gzip" else bgzfio.write_bgzf(t, cut=7001))
            ps.append(p)
        forms[form] = tuple(ps)
    forms["mixed"] = (forms["bgzf"][0], forms["gzip"][1])
    return forms


def _read_output(p, bgzf):
    raw = open(p, "rb").read()
    if not bgzf:
        return raw
    assert raw.endswith(bgzfio.EOF_BLOCK)
    blocks = bgzfio.split(raw)
    assert blocks[-1]["isize"] == 0 and all(b["isize"] == bgzfio.BLOCK_IN for b in blocks[:-2])
    assert len(blocks) == 1 or 0 < blocks[-2]["isize"] <= bgzfio.BLOCK_IN
    return bgzfio.inflate(raw)


def test_files_of_every_form(tmp_path):
    c = sc.cases()["three_hundred"]
    d = str(tmp_path)
    for form, (p1, p2) in _write_forms(d, c).items():
        for bgzf in (False, True):
            o1, o2 = (os.path.join(d, "out_%s_%d_%d.fq" % (form, bgzf, k)) for k in (1, 2))
            st = api.fastq_standardize(p1, p2, o1, o2, bgzf=bgzf, timed=bgzf)
            print(form, bgzf, st)
            assert _read_output(o1, bgzf) == c.out1 and _read_output(o2, bgzf) == c.out2, (form, bgzf)
            assert not os.path.exists(o1 + ".tmp") and not os.path.exists(o2 + ".tmp")
            assert (st["records"], st["skipped_lines"], st["format"], st["decided_by"], st["with_barcode"], st["valid"]) == (c.n, 0, "stlfr", 0, c.with_bc, c.valid)
            assert (st["bytes_in_r1"], st["bytes_in_r2"], st["bytes_out_r1"], st["bytes_out_r2"]) == (len(c.t1), len(c.t2), len(c.out1), len(c.out2))


def test_a_bgzf_output_of_several_blocks_and_empty_outputs(tmp_path):
    c = sc.cases()["many"]
    d = str(tmp_path)
    p1, p2 = os.path.join(d, "m1.fq.gz"), os.path.join(d, "m2.fq")
    bgzfio.write_bgzf_file(p1, c.t1, level=1)
    with open(p2, "wb") as f:
        f.write(c.t2)
    o1, o2 = os.path.join(d, "s1.fq.gz"), os.path.join(d, "s2.fq.gz")
    st = api.fastq_standardize(p1, p2, o1, o2, bgzf=True)
    print(st)
    assert len(bgzfio.split(open(o1, "rb").read())) > 4
    assert _read_output(o1, True) == c.out1 and _read_output(o2, True) == c.out2
    e1, e2 = devfeed.write(d, "e1.fq", b""), devfeed.write(d, "e2.fq", c.t2)
    for bgzf in (False, True):                                             # a forced format on zero records: two empty outputs
        st = api.fastq_standardize(e1, e2, o1, o2, format="tellseq", bgzf=bgzf)
        assert st["records"] == 0 and _read_output(o1, bgzf) == b"" == _read_output(o2, bgzf)


# ---- 3. the property
def _pairs_of(batches):
    """-> [(barcode, valid, info, bases1, quals1, bases2, quals2)] per pair, as the feeder delivered them"""
    out = []
    for sb in batches:
        if sb["n_sets"] == 0:
            continue
        lens = np.frombuffer(sb["lens"], np.int32)
        boff = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
        spo, noff, coff = (np.frombuffer(sb[x], np.int64) for x in ("set_pair_off", "name_off", "barcode_off"))
        for s in range(sb["n_sets"]):
            bc = sb["barcodes"][coff[s]:coff[s + 1]]
            for p in range(int(spo[s]), int(spo[s + 1])):
                a, b, e = (int(boff[2 * p + k]) for k in range(3))
                out.append((bc, bool(sb["valid"][p]), sb["names"][noff[p]:noff[p + 1]], sb["bases"][a:b], sb["quals"][a:b], sb["bases"][b:e], sb["quals"][b:e]))
    return out


@pytest.mark.parametrize("fmt", (sc.HAPLOTAGGING, sc.STLFR, sc.TELLSEQ))
def test_the_host_feeder_reads_the_contract_from_the_output(tmp_path, fmt):
    c = sc.Case(*sc.raw_pair(fmt, 90, seed=fmt))
    assert c.found == fmt and c.with_bc == c.n == 90 and 0 < c.valid < c.n
    d = str(tmp_path)
    p1, p2 = devfeed.write(d, "raw1.fq", c.t1), devfeed.write(d, "raw2.fq", c.t2)
    o1, o2 = os.path.join(d, "std1.fq"), os.path.join(d, "std2.fq")
    st = api.fastq_standardize(p1, p2, o1, o2)
    assert st["format"] == sc.NAMES[fmt] and open(o1, "rb").read() == c.out1 and open(o2, "rb").read() == c.out2
    fd = api.Feeder(o1, o2)                                              # the host feeder is the yardstick
    got = _pairs_of(devfeed.feed_all(fd, 20))
    fd.close()
    assert len(got) == c.n
    code = lambda s: bytes(devfeed.nt4(chr(x)) for x in s)
    for g, (r1, r2, _), (ident, bc, v) in zip(got, c.recs, c.fields):
        l1, l2 = r1.split(b"\n"), r2.split(b"\n")
        assert g == (bc, bool(v), ident, code(l1[1]), l1[3], code(l2[1]), l2[3]), ident
    # the raw files give the feeder nothing to place by: no valid read (and, but for haplotagging's BX:Z:, no barcode)
    fd = api.Feeder(p1, p2)
    raw = _pairs_of(devfeed.feed_all(fd, 20))
    fd.close()
    assert not any(g[1] for g in raw) and (fmt == sc.HAPLOTAGGING or not any(g[0] for g in raw))
    # and the sort of the output orders by that barcode
    s1, s2 = os.path.join(d, "sorted1.fq"), os.path.join(d, "sorted2.fq")
    srt = api.fastq_sort(o1, o2, s1, s2)
    chk = api.fastq_sort(s1, s2, check=True)
    assert chk["runs"] == chk["distinct"] == srt["distinct"] == len({f[1] for f in c.fields}) and chk["records"] == c.n


# ---- 4. detection alone, and a pair that is standard already
def test_detection_and_a_standard_pair(tmp_path):
    d = str(tmp_path)
    out = os.path.join(d, "out")
    os.mkdir(out)
    o1, o2 = os.path.join(out, "o1.fq"), os.path.join(out, "o2.fq")
    cs = sc.cases()
    for name, want in (("hap_auto", "haplotagging"), ("stlfr_auto", "stlfr"), ("tell_auto", "tellseq"), ("det_hap_vx", "standard"), ("det_plain", "unknown"), ("det_199", "stlfr"),
                       ("det_200", "unknown"), ("empty", "unknown")):
        c = cs[name]
        p1, p2 = devfeed.write(d, name + "_1.fq", c.t1), devfeed.write(d, name + "_2.fq", c.t2)
        st = api.fastq_standardize(p1, p2, detect=True)
        assert (st["format"], st["decided_by"], st["records"]) == (want, c.decided, 0) and sc.NAMES[c.found] == want, name
        st = api.fastq_standardize(p1, p2, o1, o2, format="stlfr", detect=True)      # detection only, whatever else is passed
        assert st["format"] == want and os.listdir(out) == [], name
    c = cs["det_hap_vx"]
    p1, p2 = os.path.join(d, "det_hap_vx_1.fq"), os.path.join(d, "det_hap_vx_2.fq")
    st = api.fastq_standardize(p1, p2, o1, o2)                            # "auto" on a standard pair: nothing is written, no file is made
    assert st["format"] == "standard" and st["records"] == 0 and st["bytes_out_r1"] == 0 and os.listdir(out) == []
    r1, r2, st = e2e.standardize(p1, p2, os.path.join(d, "out_e2e"))
    assert (r1, r2) == (p1, p2) and not st["standardized"] and not os.path.exists(os.path.join(d, "out_e2e"))
    f = cs["hap_vx_forced"]
    r1, r2, st = e2e.standardize(p1, p2, os.path.join(d, "out_e2e"), format="haplotagging", bgzf=True)     # a forced format converts it
    assert st["standardized"] and r1 != r2 and _read_output(r1, True) == f.out1 and _read_output(r2, True) == f.out2
    c = cs["tell_auto"]
    r1, r2, st = e2e.standardize(os.path.join(d, "tell_auto_1.fq"), os.path.join(d, "tell_auto_2.fq"), os.path.join(d, "out_e2e"))
    assert st["standardized"] and st["format"] == "tellseq" and open(r1, "rb").read() == c.out1 and open(r2, "rb").read() == c.out2
    with pytest.raises(api.ArachneError) as e:
        e2e.standardize(os.path.join(d, "det_plain_1.fq"), os.path.join(d, "det_plain_2.fq"), os.path.join(d, "out_e2e"))
    assert e.value.code == api.ARX_E_ARG


# ---- 5. what is refused
def test_what_is_refused_leaves_nothing_behind(tmp_path):
    d = str(tmp_path)
    c = sc.cases()["three_hundred"]
    forms = _write_forms(d, c)
    p1, p2 = forms["bgzf"]
    out = os.path.join(d, "out")
    os.mkdir(out)
    o1, o2 = os.path.join(out, "o1.fq"), os.path.join(out, "o2.fq")

    def refused(code, *a, **kw):
        with pytest.raises(api.ArachneError) as e:
            api.fastq_standardize(*a, **kw)
        assert e.value.code == code, str(e.value)
        assert os.listdir(out) == []                                     # neither an output nor a .tmp
        return str(e.value)

    u = sc.cases()["det_200"]
    u1, u2 = devfeed.write(d, "u1.fq", u.t1), devfeed.write(d, "u2.fq", u.t2)
    msg = refused(api.ARX_E_ARG, u1, u2, o1, o2)                           # unknown under "auto"
    assert "200" in msg and "format" in msg
    for fmt in (4, 5, 9):
        refused(api.ARX_E_ARG, p1, p2, o1, o2, format=fmt)
    raw = bytearray(open(p1, "rb").read())
    blocks = bgzfio.split(bytes(raw))
    assert len(blocks) > 3
    raw[blocks[2]["at"] + blocks[2]["size"] - 8] ^= 0x55                 # a CRC that does not match: a status of the inflate kernel
    bad = os.path.join(d, "badcrc.fq.gz")
    with open(bad, "wb") as f:
        f.write(raw)
    assert "inflate" in refused(api.ARX_E_IO, bad, p2, o1, o2, format="stlfr")
    refused(api.ARX_E_IO, os.path.join(d, "no_such_file.fq"), p2, o1, o2)
    refused(api.ARX_E_IO, p1, os.path.join(d, "no_such_file.fq"), detect=True)
    not_a_dir = os.path.join(d, "in_plain_1.fq", "o1.fq")               # under a regular file: unwritable whoever runs the test
    refused(api.ARX_E_IO, p1, p2, not_a_dir, o2)
    refused(api.ARX_E_IO, p1, p2, o1, not_a_dir)
    if os.geteuid() != 0:
        locked = os.path.join(d, "locked")
        os.mkdir(locked, 0o500)
        refused(api.ARX_E_IO, p1, p2, os.path.join(locked, "o1.fq"), o2)
        assert os.listdir(locked) == []
    for a in forms["plain"]:
        refused(api.ARX_E_ARG, *forms["plain"], a, o2)                   # an output path that is an input
        refused(api.ARX_E_ARG, *forms["plain"], o1, os.path.join(d, ".", os.path.basename(a)))
    refused(api.ARX_E_ARG, p1, p2, o1, o1)
    refused(api.ARX_E_ARG, p1, p2, None, o2)
    lib = api._load(api.LIB_PATH)
    fn = api._selftest_fn(lib, "arx_fastq_standardize")
    import ctypes as C
    msg_buf = C.create_string_buffer(256)
    for flags in (4, 0x200, 0x80):
        assert fn(0, p1.encode(), p2.encode(), o1.encode(), o2.encode(), 0, flags, None, msg_buf, 256) == api.ARX_E_ARG and b"flag" in msg_buf.value
    assert os.listdir(out) == []
    # the inputs are as they were, and the process converts a good file afterwards
    assert open(forms["plain"][0], "rb").read() == c.t1 and open(forms["plain"][1], "rb").read() == c.t2
    st = api.fastq_standardize(p1, p2, o1, o2)
    assert st["records"] == c.n and open(o1, "rb").read() == c.out1 and open(o2, "rb").read() == c.out2
    assert sorted(os.listdir(out)) == ["o1.fq", "o2.fq"]

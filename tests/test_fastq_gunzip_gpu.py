"""GPU test of ARX_FQSORT_GUNZIP_DEVICE / ARX_FQSTD_GUNZIP_DEVICE (gunzip="device" in api.py): the same small pair as plain text, as gzip and as
gzip of several members goes through the four file-pair calls with the chunked gzip inflate on the device and with zlib on the reader threads,
which is what the calls did before the flag existed.  The output files must be the same bytes and the first twelve statistics the same numbers.
A damaged gzip file is ARX_E_IO and leaves nothing behind; a BGZF and a plain input go the way they go without the flag."""
import gzip
import os

import numpy as np
import pytest

import bgzfio
import fqstdcases as sc
from arachne_amd import api

pytestmark = pytest.mark.gpu
ARX_E_IO = -5
RUN = 65536                      # run_bytes of the calls that sort in runs: a few runs of this pair
FORMS = ("plain", "gzip", "members")
SAME_SORT = api._FQSORT_STATS[:12]
SAME_STD = api._FQSTD_STATS[:12]
GZ = dict(plain=0, gzip=None, members=None)      # gzip files a call with gunzip="device" must hand to the device: none, or at least one


def _forms(d, stem, t1, t2):
    """the two texts as plain files, as gzip files and as gzip files of three members cut at any byte -> {form: (r1, r2)}"""
    out = {}
    for form in FORMS:
        ps = []
        for k, t in enumerate((t1, t2)):
            cut = (len(t) // 2 + 17, len(t) // 2 + 17 + len(t) // 3)
            data = t if form == "plain" else gzip.compress(t, 6) if form == "gzip" else gzip.compress(t[:cut[0]], 1) + gzip.compress(t[cut[0]:cut[1]], 9) + gzip.compress(t[cut[1]:], 6)
            p = os.path.join(d, "%s_%s_%d.fq%s" % (stem, form, k + 1, "" if form == "plain" else ".gz"))
            with open(p, "wb") as f:
                f.write(data)
            ps.append(p)
        out[form] = tuple(ps)
    return out


def _random_reads(text, seed):
    """the same records with random bases and qualities of the same lengths: text that compresses the way reads do, not thirty times"""
    rng = np.random.default_rng(seed)
    lines = text.split(b"\n")
    for k in range(1, len(lines), 4):
        n = len(lines[k])
        lines[k] = bytes(b"ACGT"[i] for i in rng.integers(0, 4, n))
        lines[k + 2] = bytes(int(q) for q in np.array([35, 45, 56, 70], np.uint8)[rng.choice(4, n, p=[.02, .05, .13, .8])])
    return b"\n".join(lines)


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """raw: a stLFR pair as the sequencer names it; std: the same pair standardized (by the call itself, from plain text), not yet sorted"""
    d = str(tmp_path_factory.mktemp("gunzip_pairs"))
    t1, t2 = (_random_reads(t, 31 + k) for k, t in enumerate(sc.raw_pair(sc.STLFR, 1500, seed=9, l1=100, l2=90)[:2]))
    raw = _forms(d, "raw", t1, t2)
    s1, s2 = os.path.join(d, "std1.fq"), os.path.join(d, "std2.fq")
    api.fastq_standardize(raw["plain"][0], raw["plain"][1], s1, s2)
    std = _forms(d, "std", open(s1, "rb").read(), open(s2, "rb").read())
    assert os.path.getsize(raw["gzip"][0]) > 40000           # more than one chunk of the default 32 KiB
    for kind in (raw, std):                                  # and the device takes all of these files: a pass through the host's zlib shows nothing
        for form in ("gzip", "members"):
            for p in kind[form]:
                r = api.selftest_gunzip(open(p, "rb").read(), cap=1 << 20)
                assert r["rc"] == 0 and r["fallback"] == 0 and r["host_bytes"] == 0 and r["members"] == (1 if form == "gzip" else 3), (p, r)
    return dict(raw=raw, std=std, dir=d)


def _path_taken(how, tag, gz_files):
    """the call that just ended gave the device `gz_files` gzip files (None: at least one) with gunzip="device", and none without; the host's
    zlib inflated nothing of them"""
    c = api.fastq_gunzip_counters()
    if how == "host" or gz_files == 0:
        assert c == dict(files=0, launches=0, accepted=0, bytes=0, host_bytes=0, fallbacks={}), (tag, c)
    else:
        assert (c["files"] >= 1 if gz_files is None else c["files"] == gz_files) and c["launches"] >= c["files"] and c["accepted"] >= c["launches"], (tag, c)
        assert c["bytes"] > 0 and c["host_bytes"] == 0 and c["fallbacks"] == {}, (tag, c)


def _both(call, out_dir, tag, same, gz_files=None, **kw):
    """the call with gunzip="host" and with gunzip="device": the same files, the same first statistics -> the host's stats"""
    got = {}
    for how in ("host", "device"):
        o1, o2 = (os.path.join(out_dir, "%s_%s_%d.out" % (tag, how, k)) for k in (1, 2))
        api.fastq_gunzip_counters(reset=True)
        st = call(o1, o2, gunzip=how, **kw)
        _path_taken(how, tag, gz_files)
        assert not os.path.exists(o1 + ".tmp") and not os.path.exists(o2 + ".tmp")
        got[how] = (st, open(o1, "rb").read(), open(o2, "rb").read())
        os.remove(o1), os.remove(o2)
    assert got["device"][1] == got["host"][1] and got["device"][2] == got["host"][2], tag
    assert {k: got["device"][0][k] for k in same} == {k: got["host"][0][k] for k in same}, tag
    assert got["host"][0]["records"] == 1500 and len(got["host"][1]) > 0
    return got["host"][0]


def _both_checks(call, same, gz_files=None, **kw):
    st = {}
    for how in ("host", "device"):
        api.fastq_gunzip_counters(reset=True)
        st[how] = call(None, None, gunzip=how, **kw)
        _path_taken(how, "check", gz_files)
    assert {k: st["device"][k] for k in same} == {k: st["host"][k] for k in same}
    return st["host"]


@pytest.mark.parametrize("form", FORMS)
def test_sort_and_sort_in_runs(pairs, tmp_path, form):
    p1, p2 = pairs["std"][form]
    d = str(tmp_path)
    for bgzf in (False, True):
        st = _both(lambda o1, o2, **kw: api.fastq_sort(p1, p2, o1, o2, bgzf=bgzf, **kw), d, "sort_%s_%d" % (form, bgzf), SAME_SORT, gz_files=GZ[form])
        ex = _both(lambda o1, o2, **kw: api.fastq_sort_ex(p1, p2, o1, o2, bgzf=bgzf, run_bytes=RUN, tmp_dir=d, **kw), d, "ex_%s_%d" % (form, bgzf), SAME_SORT, gz_files=GZ[form])
        assert ex["sorted_runs"] >= 2 and st["bytes_out_r1"] == st["bytes_in_r1"]         # a few runs
    chk = _both_checks(lambda o1, o2, **kw: api.fastq_sort(p1, p2, o1, o2, check=True, **kw), SAME_SORT, gz_files=GZ[form])
    assert chk["records"] == 1500 and chk["bytes_out_r1"] == 0
    _both_checks(lambda o1, o2, **kw: api.fastq_sort_ex(p1, p2, o1, o2, check=True, run_bytes=RUN, **kw), SAME_SORT, gz_files=GZ[form])
    assert os.listdir(d) == []


@pytest.mark.parametrize("form", FORMS)
def test_standardize(pairs, tmp_path, form):
    p1, p2 = pairs["raw"][form]
    d = str(tmp_path)
    for bgzf in (False, True):
        st = _both(lambda o1, o2, **kw: api.fastq_standardize(p1, p2, o1, o2, bgzf=bgzf, **kw), d, "std_%s_%d" % (form, bgzf), SAME_STD, gz_files=GZ[form])
        assert st["format"] == "stlfr"
    det = _both_checks(lambda o1, o2, **kw: api.fastq_standardize(p1, p2, o1, o2, detect=True, **kw), SAME_STD, gz_files=GZ[form])
    assert det["format"] == "stlfr"
    assert os.listdir(d) == []


@pytest.mark.parametrize("form", FORMS)
def test_prepare(pairs, tmp_path, form):
    p1, p2 = pairs["raw"][form]
    d = str(tmp_path)
    for run_bytes in (0, RUN):
        for bgzf in (False, True):
            st = _both(lambda o1, o2, **kw: api.fastq_prepare(p1, p2, o1, o2, bgzf=bgzf, run_bytes=run_bytes, tmp_dir=d, **kw), d, "prep_%s_%d_%d" % (form, run_bytes, bgzf),
                       SAME_SORT, gz_files=GZ[form])
            assert st["format"] == "stlfr"
        _both_checks(lambda o1, o2, **kw: api.fastq_prepare(p1, p2, o1, o2, check=True, run_bytes=run_bytes, **kw), SAME_SORT, gz_files=GZ[form])
    assert os.listdir(d) == []


def test_the_outputs_of_all_forms_are_the_same_bytes(pairs, tmp_path):
    d = str(tmp_path)
    seen = set()
    for form in FORMS:
        p1, p2 = pairs["raw"][form]
        o1, o2 = os.path.join(d, "o1"), os.path.join(d, "o2")
        api.fastq_prepare(p1, p2, o1, o2, gunzip="device")
        seen.add((open(o1, "rb").read(), open(o2, "rb").read()))
    assert len(seen) == 1


def test_a_damaged_gzip_file_is_an_io_error_and_leaves_nothing(pairs, tmp_path):
    d = str(tmp_path)
    bad = {}
    for kind in ("std", "raw"):                              # R2 with one bit flipped behind the middle
        bad[kind] = os.path.join(d, "bad_%s_2.fq.gz" % kind)
        raw = bytearray(open(pairs[kind]["gzip"][1], "rb").read())
        raw[len(raw) * 6 // 10] ^= 0x10
        with open(bad[kind], "wb") as f:
            f.write(bytes(raw))
    std1, raw1 = pairs["std"]["gzip"][0], pairs["raw"]["gzip"][0]
    o1, o2 = os.path.join(d, "o1.fq"), os.path.join(d, "o2.fq")
    for how in ("host", "device"):
        for call in (lambda: api.fastq_sort(std1, bad["std"], o1, o2, gunzip=how), lambda: api.fastq_sort_ex(std1, bad["std"], o1, o2, run_bytes=RUN, tmp_dir=d, gunzip=how),
                     lambda: api.fastq_standardize(raw1, bad["raw"], o1, o2, format="stlfr", gunzip=how),
                     lambda: api.fastq_prepare(raw1, bad["raw"], o1, o2, format="stlfr", gunzip=how), lambda: api.fastq_sort(std1, bad["std"], check=True, gunzip=how)):
            with pytest.raises(api.ArachneError) as e:
                call()
            assert e.value.code == ARX_E_IO, how
            assert sorted(os.listdir(d)) == ["bad_raw_2.fq.gz", "bad_std_2.fq.gz"], how


def test_bgzf_and_plain_inputs_go_as_they_go_without_the_flag(pairs, tmp_path):
    d = str(tmp_path)
    t1, t2 = (open(p, "rb").read() for p in pairs["std"]["plain"])
    b1, b2 = os.path.join(d, "in1.fq.gz"), os.path.join(d, "in2.fq.gz")
    for p, t in ((b1, t1), (b2, t2)):
        with open(p, "wb") as f:
            f.write(bgzfio.write_bgzf(t, cut=7001))
    for (p1, p2), n_gz in (((b1, b2), 0), (pairs["std"]["plain"], 0), ((b1, pairs["std"]["gzip"][1]), 1)):     # (the last: R1 BGZF, R2 gzip -- each file by itself)
        _both(lambda o1, o2, **kw: api.fastq_sort(p1, p2, o1, o2, **kw), d, "as_before", SAME_SORT, gz_files=n_gz)
    assert sorted(os.listdir(d)) == ["in1.fq.gz", "in2.fq.gz"]


def test_an_unknown_keyword_value_is_refused(pairs):
    with pytest.raises(ValueError):
        api.fastq_sort(*pairs["std"]["gzip"], check=True, gunzip="gpu")

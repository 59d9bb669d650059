"""What the four FASTQ file-pair calls refuse, and in which words (arx_fastq_sort, arx_fastq_sort_ex, arx_fastq_standardize, arx_fastq_prepare;
arachne_amd/csrc/arx_bgzf.hip, hip_fqsort.h, hip_fqstd.h, hip_fqprep.h).  run(d) makes every refusal once through the C ABI and returns
{call: {case: {"code": the call's return value, "msg": the text}}}, the directory d in every text replaced by <d>.
tests/test_fastq_refusals_gpu.py holds the result to tests/golden/fastq_refusals.json.

That file is a record of what the calls said before their host plumbing was folded into one path: `python tests/fqrefusalcases.py --record
[PATH]` writes it from the library that is built, so it is run on the commit whose texts are to be kept and never on the code under test.

The inputs are the neighbouring tests': three_hundred (fqsortcases.py for the sorts, fqstdcases.py for the standardization), run_borders and
std_det_200 (fqprepcases.py), too_long (fqextcases.py); runs of 4096 bytes.  arx_fastq_prepare is asked in core (run_bytes 0) and in runs
wherever a file is touched, since the two read and write through different code."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fastq_refusals.json")
RUN = 4096
CALLS = ("sort", "sort_ex", "standardize", "prepare")
HAS_RUNS, HAS_FORMAT, HAS_MAX = ("sort_ex", "prepare"), ("standardize", "prepare"), ("sort", "sort_ex", "prepare")
STLFR = 2                                                       # ARX_FQSTD_STLFR


def call(lib, name, r1, r2, o1, o2, format=0, flags=0, max_bytes=0, run_bytes=RUN, tmp_dir=None):
    """one call through the C ABI, with the arguments it has -> (code, text)"""
    from arachne_amd import api
    enc = lambda p: None if p is None else os.fsencode(p)
    msg = C.create_string_buffer(1024)
    fn = api._selftest_fn(lib, "arx_fastq_" + name)
    a = [0, enc(r1), enc(r2), enc(o1), enc(o2)]
    if name in HAS_FORMAT:
        a.append(format)
    a.append(flags)
    if name in HAS_MAX:
        a.append(max_bytes)
    if name in HAS_RUNS:
        a += [run_bytes, enc(tmp_dir)]
    return fn(*a, None, msg, 1024), msg.value.decode(errors="replace")


def _damaged(path, to):
    """the BGZF file with one byte of the CRC of its last block of data flipped"""
    import bgzfio
    raw = bytearray(open(path, "rb").read())
    blocks = bgzfio.split(bytes(raw))
    assert len(blocks) > 1
    b = blocks[-2]
    raw[b["at"] + b["size"] - 8] ^= 0x55
    with open(to, "wb") as f:
        f.write(raw)
    return to


def run(d):
    """-> ({call: {case: {"code", "msg"}}}, {call: whether <out>/o1.fq.tmp, made as a directory before the call, was still there after it})"""
    import bgzfio
    import devfeed
    import fqextcases as xc
    import fqprepcases as pc
    import fqsortcases as fc
    import fqstdcases as sc
    from arachne_amd import api
    lib = api._load(api.LIB_PATH)
    out, tmp = os.path.join(d, "out"), os.path.join(d, "tmp")
    os.mkdir(out)
    os.mkdir(tmp)
    o1, o2 = os.path.join(out, "o1.fq"), os.path.join(out, "o2.fq")
    inputs = dict(sort=fc.cases()["three_hundred"], sort_ex=fc.cases()["three_hundred"], standardize=sc.cases()["three_hundred"], prepare=pc.cases()["run_borders"])
    u = pc.cases()["std_det_200"]
    u1, u2 = devfeed.write(d, "undetectable_1.fq", u.t1), devfeed.write(d, "undetectable_2.fq", u.t2)
    x = xc.cases()["too_long"]
    l1, l2 = devfeed.write(d, "too_long_1.fq", x.case.t1), devfeed.write(d, "too_long_2.fq", x.case.t2)
    a_file = devfeed.write(d, "a_file", b"not a directory\n")
    missing = os.path.join(d, "no_such_file.fq")
    got, kept = {}, {}
    for name in CALLS:
        c = inputs[name]
        p1, p2 = devfeed.write(d, name + "_1.fq", c.t1), devfeed.write(d, name + "_2.fq", c.t2)
        z1 = os.path.join(d, name + "_1.fq.gz")
        with open(z1, "wb") as f:
            f.write(bgzfio.write_bgzf(c.t1, cut=7001))
        bad = _damaged(z1, os.path.join(d, name + "_badcrc.fq.gz"))
        fmt = STLFR if name in HAS_FORMAT else 0                # the cases' own format, so that only what is refused is at work
        r = {}

        def ask(case, *a, **kw):
            kw.setdefault("tmp_dir", tmp)
            kw.setdefault("format", fmt)
            code, msg = call(lib, name, *a, **kw)
            assert code != 0, (name, case)
            assert os.listdir(tmp) == [] and [e for e in os.listdir(out) if e != "o1.fq.tmp"] == [], (name, case)     # nothing is left behind
            r[case] = dict(code=code, msg=msg.replace(d, "<d>"))

        ask("unknown_flag", p1, p2, o1, o2, flags=0x80)
        ask("null_output", p1, p2, None, o2)
        ask("same_output_twice", p1, p2, o1, o1)
        ask("output_is_an_input", p1, p2, o1, os.path.join(d, ".", os.path.basename(p2)))
        if name in HAS_FORMAT:
            ask("bad_format", p1, p2, o1, o2, format=5)
            ask("undetectable", u1, u2, o1, o2, format=0)
        if name in HAS_RUNS:
            ask("run_bytes_minus_two", p1, p2, o1, o2, run_bytes=-2)
            ask("run_bytes_under_the_window", p1, p2, o1, o2, run_bytes=fc.MIN_WINDOW - 1)
            ask("tmp_dir_under_a_file", p1, p2, o1, o2, tmp_dir=os.path.join(a_file, "t"))
            ask("record_longer_than_a_run", l1, l2, o1, o2, run_bytes=fc.MIN_WINDOW)
        for tag, rb in (("", RUN), ("_in_core", 0)) if name == "prepare" else (("", RUN),):
            ask("missing_input" + tag, missing, p2, o1, o2, run_bytes=rb)
            ask("missing_second_input" + tag, p1, missing, o1, o2, run_bytes=rb)
            ask("output_under_a_file" + tag, p1, p2, os.path.join(a_file, "o1.fq"), o2, run_bytes=rb)
            ask("second_output_under_a_file" + tag, p1, p2, o1, os.path.join(a_file, "o2.fq"), run_bytes=rb)
            ask("flipped_crc" + tag, bad, p2, o1, o2, run_bytes=rb)
            if name in HAS_MAX:
                ask("max_bytes_one_short" + tag, p1, p2, o1, o2, max_bytes=len(c.t1) + len(c.t2) - 1, run_bytes=rb)
        # <out>/o1.fq.tmp is a directory: fopen fails on it, and the call did not make it
        os.mkdir(o1 + ".tmp")
        ask("tmp_name_is_a_directory", p1, p2, o1, o2)
        kept[name] = os.path.isdir(o1 + ".tmp")
        if kept[name]:
            os.rmdir(o1 + ".tmp")
        got[name] = r
    return got, kept


if __name__ == "__main__":
    import tempfile
    sys.path.insert(0, os.path.dirname(HERE))
    if len(sys.argv) not in (2, 3) or sys.argv[1] != "--record":
        sys.exit("usage: fqrefusalcases.py --record [PATH]    (on the commit whose texts are to be kept; PATH: tests/golden/fastq_refusals.json)")
    path = sys.argv[2] if len(sys.argv) == 3 else GOLDEN
    with tempfile.TemporaryDirectory(prefix="arx_refusals_") as d:
        got, kept = run(d)
    with open(path, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d refusals" % (path, sum(len(v) for v in got.values())))
    print("o1.fq.tmp, a directory before the call, was still there after it:", kept)

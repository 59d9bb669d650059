"""GPU tests of the FASTA pack (arachne_amd/csrc/dev_fapack.h, hip_fapack.h behind arx_index_build_ex and arx_selftest_fasta_pack): every case of
fapackcases.py through the product's kernels at three window sizes against the restatement; the seeded genomes of test_index_build_gpu.py as
plain text, gzip and BGZF (blocks cut every 4,093 bytes, inside lines, headers and holes) against arx_index_build's files of the plain text
and the reference's (oracle/_ref live, or its digests in tests/golden/ref_live_v1.npz); one full build from BGZF with small sort chunks; a
single-line FASTA; and the refusals, each with its code and text and with nothing left behind."""
import filecmp
import gzip
import hashlib
import os

import numpy as np
import pytest

import bgzfio
import fapackcases as fc
import refdrv
import workloads
from arachne_amd import api

pytestmark = pytest.mark.gpu
EXTS = ("bwt", "sa", "pac", "ann", "amb")
PACK_EXTS = ("pac", "ann", "amb")
BLOCK = 4093


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _genome(case):
    if case == "three_contigs":
        return workloads.nasty_genome(5, contig_lens=(1000003, 777, 50021), alt_contigs=0)
    return workloads.nasty_genome(7, contig_lens=(300000,), alt_contigs=0)


class Forms:
    """one seeded genome as plain text, gzip and BGZF; arx_index_build's files of the plain text (host.*); the reference's files or digests"""

    def __init__(self, case, d):
        self.case, self.dir, self.g = case, d, _genome(case)
        self.plain = os.path.join(d, "g.fa")
        self.g.write_fasta(self.plain)
        text = open(self.plain, "rb").read()
        self.gz, self.bgzf = os.path.join(d, "g.fa.gz"), os.path.join(d, "g.bgzf.fa.gz")
        with open(self.gz, "wb") as f:
            f.write(gzip.compress(text, 6))
        bgzfio.write_bgzf_file(self.bgzf, text, cut=BLOCK)
        self.host = os.path.join(d, "host")
        old = os.environ.get("ARX_INDEX_HOST")
        os.environ["ARX_INDEX_HOST"] = "1"                              # the yardstick's suffix sort is not under test here
        try:
            api.index_build(self.plain, self.host)
        finally:
            if old is None:
                os.environ.pop("ARX_INDEX_HOST")
            else:
                os.environ["ARX_INDEX_HOST"] = old
        self.ref, self.digests = None, None
        if refdrv.available():
            self.ref = os.path.join(d, "ref")
            assert refdrv.Ref().index_build(self.plain, self.ref) == 0
        else:
            z = np.load(os.path.join(workloads.GOLDEN_DIR, "ref_live_v1.npz"))
            key = "gpuidx_" + case
            assert _sha(self.plain) == str(z[key + "_fasta"]), "the seeded genome differs from the one the fixture was made from (numpy version?)"
            self.digests = {ext: str(z[key + "_" + ext]) for ext in EXTS}

    def hold(self, prefix, exts):
        for ext in exts:
            assert filecmp.cmp(self.host + "." + ext, prefix + "." + ext, shallow=False), (self.case, prefix, ext)
            if self.ref is not None:
                assert filecmp.cmp(self.ref + "." + ext, prefix + "." + ext, shallow=False), (self.case, prefix, ext)
            else:
                assert _sha(prefix + "." + ext) == self.digests[ext], (self.case, prefix, ext)


@pytest.fixture(scope="module")
def nasty(tmp_path_factory):
    return Forms("nasty", str(tmp_path_factory.mktemp("fapack_nasty")))


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    return Forms("three_contigs", str(tmp_path_factory.mktemp("fapack_three")))


def _left_behind(d, before):
    return sorted(set(os.listdir(d)) - set(before))


# ---- 1. the cases against the restatement
def test_the_cases_are_what_they_claim():
    fc.check_cases()


@pytest.mark.parametrize("window", fc.WINDOWS)
def test_every_case_at_every_window(window):
    for name, c in fc.cases().items():
        g = api.selftest_fasta_pack(c.text, window_bytes=window)
        if c.status != fc.OK:
            assert (g["rc"], g["refused"]) == (api.ARX_E_OPEN, c.status), (name, window)
            continue
        assert g["rc"] == 0 and g["windows"] == -(-len(c.text) // window), (name, window)
        assert (g["l_pac"], g["n_amb"], g["cnt_fwd"]) == (c.l_pac, c.n_amb, c.cnt), (name, window)
        assert g["pac"] == c.pac, (name, window)
        assert g["contigs"] == c.contigs and g["holes"] == c.holes, (name, window)


def test_the_default_window_and_the_arguments():
    c = fc.cases()["many"]
    g = api.selftest_fasta_pack(c.text)
    assert g["rc"] == 0 and g["windows"] == 1 and g["pac"] == c.pac and g["holes"] == c.holes and g["contigs"] == c.contigs
    for window in (63, (1 << 24) + 1, -1):
        with pytest.raises(api.ArachneError) as e:
            api.selftest_fasta_pack(c.text, window_bytes=window)
        assert e.value.code == api.ARX_E_ARG


# ---- 2. files
@pytest.mark.parametrize("form", ["plain", "gz", "bgzf"])
def test_pack_only_of_every_form_is_the_host_builders_and_the_references(nasty, three, form):
    for f in (nasty, three):
        prefix = os.path.join(f.dir, "ex_" + form)
        st = api.index_build(getattr(f, form), prefix, pack="device", pack_only=True)
        f.hold(prefix, PACK_EXTS)
        assert not os.path.exists(prefix + ".bwt") and not os.path.exists(prefix + ".sa") and not [x for x in os.listdir(f.dir) if x.endswith(".tmp")]
        assert st["l_pac"] == sum(len(s) for s in f.g.seqs) and st["contigs"] == len(f.g.seqs) and st["holes"] > 0 and st["ambiguous"] >= st["holes"]
        assert st["text_bytes"] == os.path.getsize(f.plain) and st["compressed_bytes"] == os.path.getsize(getattr(f, form)) and st["windows"] >= 1 and st["sort_us"] == 0


def test_full_build_from_bgzf_is_the_references(nasty):
    old = {k: os.environ.get(k) for k in ("ARX_INDEX_CHUNK", "ARX_INDEX_SLICE", "ARX_INDEX_VERIFY")}
    os.environ.update(ARX_INDEX_CHUNK="20000", ARX_INDEX_SLICE="3000", ARX_INDEX_VERIFY="1")
    prefix = os.path.join(nasty.dir, "full")
    try:
        st = api.index_build(nasty.bgzf, prefix, pack="device")
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    nasty.hold(prefix, EXTS)
    assert st["sort_us"] > 0 and not [x for x in os.listdir(nasty.dir) if x.endswith(".tmp")]


# ---- 3. one line of 300,000 bases
def test_a_single_line_fasta_packs_like_the_80_column_form(nasty, tmp_path):
    fa = str(tmp_path / "one_line.fa")
    nasty.g.write_fasta(fa, width=300000)
    assert open(fa, "rb").read().count(b"\n") == 2
    api.index_build(fa, fa, pack="device", pack_only=True)
    nasty.hold(fa, PACK_EXTS)


# ---- 4. refusals: the code, the text, nothing left behind
def _refused(fasta, prefix, code, text, device=0):
    d = os.path.dirname(prefix)
    before = os.listdir(d) if os.path.isdir(d) else []
    with pytest.raises(api.ArachneError) as e:
        api.index_build(fasta, prefix, pack="device", pack_only=True, device=device)
    assert e.value.code == code and text in str(e.value), (e.value.code, str(e.value))
    if os.path.isdir(d):
        assert _left_behind(d, before) == []


def test_refusals(nasty, tmp_path):
    d = str(tmp_path)
    out = os.path.join(d, "out")
    raw = bytearray(open(nasty.bgzf, "rb").read())
    blocks = bgzfio.split(bytes(raw))
    at = blocks[3]["at"] + 18                                           # the fourth block's DEFLATE stream: its first bytes no longer say what follows
    raw[at:at + 64] = b"\xff" * 64
    damaged = os.path.join(d, "damaged.fa.gz")
    with open(damaged, "wb") as f:
        f.write(raw)
    _refused(damaged, out, api.ARX_E_IO, "BGZF")
    cut = os.path.join(d, "cut.fa.gz")
    with open(cut, "wb") as f:
        f.write(open(nasty.gz, "rb").read()[:os.path.getsize(nasty.gz) // 2])
    _refused(cut, out, api.ARX_E_IO, "read error")
    bad = os.path.join(d, "bad.fa")
    with open(bad, "wb") as f:
        f.write(fc.cases()["bad_start"].text)
    _refused(bad, out, api.ARX_E_OPEN, fc.REFUSALS[fc.BAD_START])
    empty = os.path.join(d, "empty.fa")
    open(empty, "wb").close()
    _refused(empty, out, api.ARX_E_OPEN, fc.REFUSALS[fc.EMPTY])
    _refused(os.path.join(d, "missing.fa"), out, api.ARX_E_IO, "cannot read")
    _refused(nasty.plain, os.path.join(d, "no_such_dir", "out"), api.ARX_E_IO, "cannot write")
    _refused(nasty.plain, out, api.ARX_E_DEVICE, "no such HIP device", device=4096)
    assert not [x for x in os.listdir(d) if x.startswith("out")]

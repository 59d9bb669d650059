"""CPU differential test: oracle restatement vs the reference's own C core on freshly seeded nasty workloads -- against what the
reference computed for them (tests/golden/ref_live_v1.npz, make_ref_live_golden.py) and, where oracle/_ref/libbwaref.so is
present, against the reference compiled in place, live."""
import os
import tempfile

import numpy as np
import pytest

import refdrv
import workloads

REF_LIVE = os.path.join(workloads.GOLDEN_DIR, "ref_live_v1.npz")
KEYS = ("reg_off", "regs", "alns", "cigars")


def pair_path_inputs(seed):
    """The seeded genome and reads of one case (the fixture generator runs the reference on the same ones)."""
    g = workloads.nasty_genome(seed, contig_lens=(120000, 70000, 30000), alt_contigs=2)
    rs = workloads.nasty_reads(seed, g, n_barcodes=4, pairs_per_barcode=400)
    return g, rs


@pytest.mark.parametrize("seed", [1, 2])
def test_pair_path_matches_reference(built, seed):
    import oradrv
    from test_index_build import INDEX_EXTS, sha256
    z = np.load(REF_LIVE)
    g, rs = pair_path_inputs(seed)
    tmp = tempfile.mkdtemp(prefix="arx_diff_")
    prefix = os.path.join(tmp, "g.fa")
    g.write_fasta(prefix)
    g.write_alt(prefix + ".alt")
    r = None
    if refdrv.available():
        r = refdrv.Ref()
        r.index_build(prefix, prefix)
        r.open(prefix)
    else:   # the product's builder writes the reference's index byte for byte (test_index_build.py)
        import __graft_entry__ as ge
        from arachne_amd import api
        ge.build_product()
        api.index_build(prefix, prefix)
    for ext in INDEX_EXTS:
        assert sha256(prefix + "." + ext) == str(z["pair%d_idx_%s" % (seed, ext)]), ext
    o = oradrv.Oracle(prefix)
    B = o.batch(rs.seqs, rs.lens, n_threads=2)
    A = {key: z["pair%d_%s" % (seed, key)].astype(B[key].dtype) for key in KEYS}
    if r is not None:
        live = r.batch(rs.seqs, rs.lens, n_threads=2)
        for key in KEYS:
            assert live[key].shape == A[key].shape and (live[key] == A[key]).all(), key
    for key in KEYS:
        assert A[key].shape == B[key].shape and (A[key] == B[key]).all(), key
    assert A["regs"].shape[0] > 2000
    if r is not None:
        r.close()
    o.close()


def test_chain2aln_on_the_planted_chains_matches_reference(built):
    """ora_chain2aln against the reference's own mem_chain2aln (ref_chain2aln) on every planted read of tests/extcases.py, region for region and
    bit for bit; both entry points refuse the same rows.  Runs where oracle/_ref can be built; tests/test_oracle_golden.py holds the same regions
    from the committed fixture elsewhere."""
    import subprocess
    import extcases
    import oradrv
    refdrv.need("ref_chain2aln")
    sim = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "libarx_hostsim.so")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(sim)])
    c = extcases.build_all()
    fa = c["genome"].write_index(sim)
    o, r = oradrv.Oracle(fa), refdrv.Ref(fa)
    n = n_regs = 0
    for b in c["batches"] + [c["big"]]:
        b.rows()
        for rd in b.reads:
            a = o.chain2aln(rd["read"], rd["ch"], rd["sd"], extcases.FRAC_REP_BITS)
            e = r.chain2aln(rd["read"], rd["ch"], rd["sd"], extcases.FRAC_REP_BITS)
            assert a is not None and e is not None and a[0].shape == e.shape and (a[0] == e).all(), (b.name, rd["name"])
            n += 1
            n_regs += len(e)
    assert n > 3800 and n_regs > 4000
    read = c["genome"].seqs[0][1000:1150]
    for ch, sd in (([[1040, 1, 1, 0, 30, 3, -1, 0]], [[1040, 40, 30, 30]]), ([[1040, 0, 1, 0, 30, 3, -1, 0]], [[1040, 130, 30, 30]]),
                   ([[1040, 0, 1, 0, 30, 3, -1, 0]], [[int(c["genome"].off[1]) - 10, 40, 30, 30]])):
        assert o.chain2aln(read, ch, sd) is None and r.chain2aln(read, ch, sd) is None
    o.close()
    r.close()

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

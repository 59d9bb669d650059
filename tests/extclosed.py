"""What the ARX_EXT_CLOSED tests share (test_ext_closed_hostsim.py, test_ext_closed_gpu.py): the benchmark-like read set and the on/off run."""
import numpy as np

from arachne_amd import synth

BENCH_SEED = 20250908


def bench_like_inputs():
    """10,010 pairs by the benchmark's read recipe (0.5 % substitutions, 0.02 % indels) on a 4 Mb genome with repeat families."""
    g = synth.make_genome(BENCH_SEED, [3_000_000, 1_000_000], repeat_families=[(13, 300, 0.12), (2, 6000, 0.05)])
    rs = synth.make_reads(BENCH_SEED + 1000, g, 130, 77, molecules_per_barcode=4)
    return g, rs


def run_both_ways(ref, seqs, lens, monkeypatch, keep=False):
    """The batch with ARX_EXT_CLOSED=0 and with the default: (results, counts[, batch]) each.  The switch is read when the handle is created."""
    out = []
    for closed in (False, True):
        if closed:
            monkeypatch.delenv("ARX_EXT_CLOSED", raising=False)
        else:
            monkeypatch.setenv("ARX_EXT_CLOSED", "0")
        b = ref.batch(seqs, lens).run()
        out.append((b.fetch(), b.counts(), b))
        if not (keep and closed):
            b.free()
    monkeypatch.delenv("ARX_EXT_CLOSED", raising=False)
    return out


def assert_same_results(off, on):
    for k in ("reg_off", "regs", "alns", "cigars"):
        assert np.asarray(off[k]).tobytes() == np.asarray(on[k]).tobytes(), k

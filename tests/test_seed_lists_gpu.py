"""The list passes of the seeding stage by 16-lane groups (hip_seed_lists.h: seed_merge, occ_fill) against the restatement and against their
thread-per-read forms (-m gpu).

A group holds one read's list, entry j in lane j; a read with more than 16 entries is left to the group's first lane, which runs the
thread-per-read functor.  So the edges are list lengths 0, 1, 15, 16, 17 and far above, intervals with 500 and 501 occurrences (the cap of
occ_fill, where the stride between rows starts to matter), the last group of a wavefront and the last wavefront of a launch (batches of 2, 6,
10 and 64 + 2 reads: a batch is pairs of mates, so an odd number of reads cannot be run); read lengths either side of a word of the packed rows (8 bases), reads
shorter than a seed and reads of N only ride along.

The reads are chosen from the restatement (seedcheck.Expected) before the device is looked at, and every class is asserted non-empty.  Each
batch runs once with ARX_SEED_LISTS=0 and once with the default; both are compared with the restatement interval for interval and chain by
chain, seed by seed, and with each other byte for byte (what debug_intv / debug_chains return for the live entries: beyond a list's end both
hold whatever the arena held).

Not here: a third-pass list of 16 entries (CAP_STRAT) -- a hit consumes 20 bases, a read of 255 bases yields at most 12."""
import os
import tempfile

import numpy as np
import pytest

import seedcheck
import workloads
from arachne_amd import api

pytestmark = pytest.mark.gpu

UNIT, STRIDE = 40, 60
FAMILIES = (500, 501, 1100)           # copies of three planted units: at the cap of occ_fill, one above it (stride 1), above twice the cap (stride 2)
BATCHES = (2, 6, 10, 66)              # reads come in mates (arx_batch_create takes an even number): none a multiple of the 4 reads of a wavefront or the 16 of a workgroup


def _workload(seed=5):
    """A repeat-rich genome of 340 kb with three planted families of exact copies, and a pool of reads to choose from."""
    rng = np.random.default_rng(9000 + seed)
    g = workloads.nasty_genome(seed, contig_lens=(220000, 90000, 30000))
    s = g.seqs[0]
    pos, units = 2000, []
    for copies in FAMILIES:
        u = rng.integers(0, 4, size=UNIT, dtype=np.uint8)
        units.append(u)
        for _ in range(copies):
            s[pos:pos + UNIT] = u
            s[pos + UNIT:pos + STRIDE] = rng.integers(0, 4, size=STRIDE - UNIT, dtype=np.uint8)
            s[pos + UNIT] = (u[0] + 1) % 4                 # a copy never runs on into the next
            s[pos - 1] = (u[-1] + 1) % 4
            pos += STRIDE
    reads, tags = [], []

    def add(r, tag):
        reads.append(np.asarray(r, dtype=np.uint8))
        tags.append(tag)
    rs = workloads.nasty_reads(seed, g, n_barcodes=4, pairs_per_barcode=100)
    for i in range(rs.seqs.shape[0]):
        add(rs.seqs[i, :rs.lens[i]], "nasty")
    for u, copies in zip(units, FAMILIES):
        add(u, "unit")
        add(workloads._rc(u), "unit")
        add(np.concatenate([rng.integers(0, 4, size=30, dtype=np.uint8), u, rng.integers(0, 4, size=30, dtype=np.uint8)]), "unit")
    c1 = g.seqs[1]
    for L in (18, 18, 19, 20, 149, 150, 151, 255):
        p = int(rng.integers(1000, len(c1) - 300))
        add(c1[p:p + L], "len%d" % L)
    for L in (19, 150, 255):
        add(np.full(L, 4, dtype=np.uint8), "allN")
    for k in range(3):       # a mismatch every 12 bases: a first-pass task at every one of them, no seed
        p = int(rng.integers(1000, len(c1) - 300))
        r = c1[p:p + 255].copy()
        at = np.arange(6 + k, 255, 12)
        r[at] = (r[at] + 1) % 4
        add(r, "many_tasks")
    for k in range(60):      # long reads over the repeat-rich parts with a few differences: many SMEMs
        sq = g.seqs[k % 2]
        p = int(rng.integers(150000 if k % 2 == 0 else 1000, len(sq) - 300))
        r = sq[p:p + 255].copy()
        m = rng.random(255) < (0.01, 0.03, 0.05)[k % 3]
        r[m] = (r[m] + 1) % 4
        add(workloads._rc(r) if k & 1 else r, "long")
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    return g, np.concatenate(reads), lens, tags


def _choose(exp, tags):
    """The 66 reads of the test, from the restatement alone: every class of the docstring, asserted non-empty, the edges first (the small
    batches are prefixes).  -> indices into the pool"""
    n, tags = exp.n, np.array(tags)
    tasks1 = np.bincount(exp.shape_read[exp.col("pass") == 1], minlength=len(n))
    live = np.arange(api.CAP_INTV)[None, :] < n[:, None]
    s = exp.iv[:, :, 2]
    classes = [
        ("a list of at least 33", n >= 33), ("a list of 16", n == 16), ("a list of 17", n == 17), ("a list of 15", n == 15), ("a list of 1", n == 1),
        ("an empty list of a read long enough", (n == 0) & (exp.lens >= 19) & (tags == "nasty")),
        ("an interval of exactly 500 rows", (live & (s == 500)).any(axis=1) & (n <= 16)), ("an interval of exactly 501 rows", (live & (s == 501)).any(axis=1) & (n <= 16)),
        ("an interval above twice the cap", (live & (s > 1000)).any(axis=1) & (n <= 16)), ("an interval above the cap in a long list", (live & (s > 500)).any(axis=1) & (n > 16)),
        ("more than 16 first-pass tasks", tasks1 > 16), ("more than 16 intervals", n > 16),
        ("18 bases", exp.lens == 18), ("all N", tags == "allN"),
    ] + [("%d bases" % L, tags == "len%d" % L) for L in (19, 20, 149, 150, 151, 255)]
    order = []
    for pick in (0, 1):      # one read of every class, in the order of the list; then a second one where there is one
        for what, m in classes:
            idx = np.nonzero(m)[0]
            assert len(idx) > 0, "the pool holds no read with " + what
            if pick < len(idx) and int(idx[pick]) not in order:
                order.append(int(idx[pick]))
    order += [int(i) for i in np.nonzero(tags == "allN")[0] if int(i) not in order]
    order += [int(i) for i in np.nonzero(tags == "unit")[0] if int(i) not in order]
    assert len(order) <= BATCHES[-1], len(order)
    order += [int(i) for i in np.nonzero(tags == "nasty")[0] if int(i) not in order][:BATCHES[-1] - len(order)]
    assert len(order) == BATCHES[-1]
    return order


@pytest.fixture(scope="module")
def wl(built):
    import oradrv
    g, flat, lens, tags = _workload()
    d = tempfile.mkdtemp(prefix="arx_seed_lists_")
    fa = os.path.join(d, "g.fa")
    g.write_fasta(fa)
    api.index_build(fa, fa)
    o = oradrv.Oracle(fa)
    pool = seedcheck.Expected(o, flat, lens)
    order = _choose(pool, tags)
    off = np.concatenate([[0], np.cumsum(lens)])
    exp = seedcheck.Expected(o, np.concatenate([flat[off[r]:off[r + 1]] for r in order]), lens[order])   # the 66 reads in the chosen order
    live = np.arange(api.CAP_INTV)[None, :] < exp.n[:, None]
    s = exp.iv[:, :, 2]
    assert (live & (s == 500)).any() and (live & (s == 501)).any() and (live & (s > 1000)).any()      # the cap of occ_fill from both sides, and a stride of 2
    assert set(exp.n[:5].tolist()) >= {16, 17, 15, 1} and exp.n[0] >= 33, exp.n[:5]                   # the prefixes hold the edges
    assert {18, 19, 20, 149, 150, 151, 255} <= set(exp.lens.tolist())
    ref = api.Reference(fa)
    yield ref, exp
    ref.close()
    o.close()


def _live(b):
    """what debug_intv / debug_chains return, cut to the live entries, as bytes"""
    n, iv = b.debug_intv()
    occ_off, n_chain, ch, sd = b.debug_chains()
    ci = np.repeat(occ_off[:-1].astype(np.int64), n_chain) + (np.arange(int(n_chain.sum())) - np.repeat(np.cumsum(n_chain) - n_chain, n_chain))
    c = ch[ci]
    si = np.repeat(c["seed_off"].astype(np.int64), c["n"]) + (np.arange(int(c["n"].sum())) - np.repeat(np.cumsum(c["n"]) - c["n"], c["n"]))
    return [n.tobytes(), iv[np.arange(api.CAP_INTV)[None, :] < n[:, None]].tobytes(), occ_off.tobytes(), n_chain.tobytes(), c.tobytes(), sd[si].tobytes()]


@pytest.mark.parametrize("n_reads", BATCHES)
def test_group_forms_equal_the_restatement_and_the_thread_forms(wl, monkeypatch, n_reads):
    ref, exp = wl
    e = exp.subset(np.arange(n_reads))
    got = {}
    # the interval pool and the task array are sized for an average read; a batch of two reads chosen for their long lists is not one
    monkeypatch.setenv("ARX_SEED_POOL", "8192")
    monkeypatch.setenv("ARX_SEED_TASKS", "128")
    for lists in ("0", None):
        if lists is None:
            monkeypatch.delenv("ARX_SEED_LISTS", raising=False)
        else:
            monkeypatch.setenv("ARX_SEED_LISTS", lists)
        what = "%d reads, ARX_SEED_LISTS %s" % (n_reads, lists or "unset")
        b = ref.batch(e.flat, e.lens)
        try:
            b.run(api.STAGE_SEED)
            n_iv = e.check_intervals(b, what)
            b.run(api.STAGE_CHAIN)
            n_ch = e.check_chains(b, what)
            got[lists] = _live(b)
            print(f"\n  {what}: {n_iv} intervals, {n_ch} chains, {b.counts()['n_occ']} occurrences equal the restatement's")
        finally:
            b.free()
    names = ("n_intv", "intervals", "occ_off", "n_chain", "chains", "seeds")
    differ = [names[i] for i in range(len(names)) if got["0"][i] != got[None][i]]
    assert not differ, differ

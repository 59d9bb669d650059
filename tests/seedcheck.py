"""Whole-batch comparison of the seeding stage with the restatement (oracle/arx_oracle.c), shared by tests/test_seed_shapes_hostsim.py and
tests/test_seed_variants_gpu.py: the expected intervals, chains and work shapes are computed ONCE per workload and compared with numpy per
variant -- every read, every interval, bit for bit."""
import numpy as np

from arachne_amd import api

EDGE_LENGTHS = (16, 17, 21, 22, 32, 33, 64, 65, 128, 129)   # either side of every bin edge of k_seed_bwd_g and of k_seed_bwd_wave's 64-entry chunks


class Expected:
    """What the restatement computes for a batch: intervals per read, the shape rows of every bwt_smem1a call (oradrv.Oracle.SHAPE_FIELDS) and,
    on demand, the filtered chains."""

    def __init__(self, o, flat, lens, kf=0, k3=0):
        self.o, self.flat, self.lens = o, np.ascontiguousarray(flat, dtype=np.uint8).reshape(-1), np.asarray(lens, dtype=np.int32)
        R = len(self.lens)
        self.off = np.concatenate([[0], np.cumsum(self.lens)])
        self.n = np.zeros(R, dtype=np.int32)
        self.iv = np.zeros((R, api.CAP_INTV, 4), dtype=np.uint64)
        rows, owner = [], []
        for r in range(R):
            if self.lens[r] < 19:      # shorter than min_seed_len: mem_collect_intv finds nothing to keep, the product does not look
                continue
            sh, iv = o.seed_shapes(self.flat[self.off[r]:self.off[r + 1]], kf, k3)
            assert len(iv) <= api.CAP_INTV
            self.n[r] = len(iv)
            self.iv[r, :len(iv)] = iv
            rows.append(sh)
            owner.append(np.full(len(sh), r, dtype=np.int64))
        self.shapes = np.concatenate(rows)
        self.shape_read = np.concatenate(owner)
        self._chains = None

    def col(self, name):
        return self.shapes[:, self.o.SHAPE_FIELDS.index(name)]

    def subset(self, reads):
        """The same for a slice of the batch (reads: a sorted index array), without asking the restatement again."""
        e = object.__new__(Expected)
        e.o, e.lens = self.o, self.lens[reads]
        e.flat = np.concatenate([self.flat[self.off[r]:self.off[r + 1]] for r in reads])
        e.off = np.concatenate([[0], np.cumsum(e.lens)])
        e.n, e.iv = self.n[reads], self.iv[reads]
        m = np.isin(self.shape_read, reads)
        e.shapes, e.shape_read = self.shapes[m], np.searchsorted(reads, self.shape_read[m])
        e._chains = None
        return e

    def check_intervals(self, batch, what=""):
        n, iv = batch.debug_intv()
        if not np.array_equal(n, self.n):
            r = int(np.nonzero(n != self.n)[0][0])
            raise AssertionError(f"{what}: read {r} has {n[r]} intervals, the restatement {self.n[r]}")
        live = np.arange(api.CAP_INTV)[None, :] < self.n[:, None]
        bad = live & (iv != self.iv).any(axis=2)
        if bad.any():
            r, i = np.argwhere(bad)[0]
            raise AssertionError(f"{what}: read {r} interval {i}: got {iv[r, i]}, the restatement {self.iv[r, i]}")
        return int(self.n.sum())

    def chains(self):
        """mem_chain + mem_chain_flt per read, flattened in read order: (chains per read, chain columns, seed columns, frac_rep bits of the reads with chains)."""
        if self._chains is None:
            nc, cc, ss, fr = [], [], [], []
            for r in range(len(self.lens)):
                ec, es, f = self.o.chains(self.flat[self.off[r]:self.off[r + 1]], 1)
                nc.append(len(ec))
                if len(ec):
                    cc.append(ec[:, [0, 1, 2, 4, 5, 7]])
                    fr.append(f)
                    for i in range(len(ec)):
                        ss.append(es[ec[i][3]:ec[i][3] + ec[i][2], :3])
            self._chains = (np.array(nc, dtype=np.int64), np.concatenate(cc) if cc else np.zeros((0, 6), dtype=np.int64),
                            np.concatenate(ss) if ss else np.zeros((0, 3), dtype=np.int64), np.array(fr, dtype=np.uint32))
        return self._chains

    def check_chains(self, batch, what=""):
        nc, cc, ss, fr = self.chains()
        occ_off, n_chain, ch, sd = batch.debug_chains()
        if not np.array_equal(n_chain.astype(np.int64), nc):
            r = int(np.nonzero(n_chain != nc)[0][0])
            raise AssertionError(f"{what}: read {r} has {n_chain[r]} chains, the restatement {nc[r]}")
        starts = np.repeat(occ_off[:-1].astype(np.int64), n_chain)
        within = np.arange(len(starts)) - np.repeat(np.cumsum(n_chain) - n_chain, n_chain)
        c = ch[starts + within]
        got = np.stack([c[k].astype(np.int64) for k in ("pos", "rid", "n", "w", "kept", "is_alt")], axis=1) if len(c) else np.zeros((0, 6), dtype=np.int64)
        if not np.array_equal(got, cc):
            i = int(np.argwhere((got != cc).any(axis=1))[0][0])
            raise AssertionError(f"{what}: chain {i} of the batch: got {got[i]}, the restatement {cc[i]}")
        s_start = np.repeat(c["seed_off"].astype(np.int64), c["n"])
        s_within = np.arange(len(s_start)) - np.repeat(np.cumsum(c["n"]) - c["n"], c["n"])
        s = sd[s_start + s_within]
        gs = np.stack([s[k].astype(np.int64) for k in ("rbeg", "qbeg", "len")], axis=1) if len(s) else np.zeros((0, 3), dtype=np.int64)
        assert np.array_equal(gs, ss), f"{what}: the chains' seeds differ"
        first = (np.cumsum(n_chain) - n_chain)[n_chain > 0]
        assert np.array_equal(c["frac_rep"][first].view(np.uint32), fr), f"{what}: frac_rep differs"
        return len(cc)

    # ---- what the input makes the kernels do, from the restatement alone
    def coverage(self):
        c = self.col
        p12, p1 = c("pass") < 3, c("pass") == 1
        swept = p12 & (c("x") > 0)                     # a start inside the read: the list is swept backwards (x = 0: the longest match is the SMEM)
        n = c("fwd_n")
        out = dict(
            list_lengths_swept=set(n[swept].tolist()),
            widest_later_row=int(c("widest")[swept].max()),
            most_rows_above_16=int(c("rows16")[swept].max()),
            sweeps_above_128_ext=int((swept & (c("ext") > 128)).sum()),
            sweeps_above_64_entries=int((swept & (n > 64)).sum()),
            fwd_text=int((p1 & (c("one_depth") >= 0)).sum()), fwd_no_text=int((p1 & (c("one_depth") < 0)).sum()),
            sweep_text=int((p1 & swept & (c("tail") == 1)).sum()), sweep_no_text=int((p1 & swept & (c("tail") == 0)).sum()),
            tasks=int(p12.sum()),
        )
        for ps in (1, 2, 3):
            j = c("jump")[c("pass") == ps]
            out[f"jump{ps}"] = {k: int((j == k).sum()) for k in (-1, 0, 1, 2, 3)}
        return out

    def census(self, mid=21):
        """What Batch.seed_census() must report for this batch with the row-parallel backward kernel (hip_rt.h run_seed_bwd, hip_fm_coop.h):
        every bwt_smem1a call is one task, binned by the length of its forward list (k_bin_tasks; a start at x = 0 too); a list too long for
        64 lanes goes to k_seed_bwd_wave whatever else holds; with text mode a sweep that comes to a row of one interval with one occurrence
        (first pass) is left to the tail."""
        c = self.col
        p12, n = c("pass") < 3, c("fwd_n")
        return dict(bin16=int((p12 & (n <= 16)).sum()), bin21=int((p12 & (n > 16) & (n <= mid)).sum()), bin32=int((p12 & (n > max(16, mid)) & (n <= 32)).sum()),
                    bin64=int((p12 & (n > 32)).sum()), to_wave=int((p12 & (n > 64)).sum()),
                    to_tail=int((p12 & (c("x") > 0) & (n <= 64) & (c("tail") == 1)).sum()))

    def handed_bounds(self, budget):
        """One lane per sweep (k_seed_bwd, k_seed_bwd2; dev_fm.h BwdLane::advance_nx): a sweep stops at the first row boundary at which it has spent
        `budget` extensions and has not ended.  Rows never grow, so a sweep with more than budget + (list length) extensions is handed over
        and one with fewer than budget never is: (lower, upper) bound of the hand-offs."""
        c = self.col
        swept = (c("pass") < 3) & (c("x") > 0)
        return int((swept & (c("ext") > budget + c("fwd_n"))).sum()), int((swept & (c("ext") >= budget)).sum())

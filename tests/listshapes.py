"""What the list_shapes workload (tests/workloads.py) makes the list stages do, from the restatement alone (ora_list_shapes: counts taken inside
mem_chain, mem_chain_flt, mem_sort_dedup_patch, mem_patch_reg and mem_matesw while one pair runs).  tests/test_list_shapes_hostsim.py asserts the
shape conditions from it; tests/test_wave_lists_gpu.py derives from it which reads and pairs the wavefront-per-item kernels must have taken."""
import numpy as np

# pipeline.h, restated: the thresholds and caps of the heavy-item hand-over
CHAIN_HEAVY_MIN, CHAIN_LDS_SMALL, CHAIN_LDS_OCC = 64, 256, 832
DEDUP_HEAVY_MIN, DEDUP_LDS_REGS = 32, 256
RESCUE_HEAVY_MIN, RESCUE_LDS_REGS, MAX_RESCUE = 48, 680, 50


def pair_cap(n0, n1):
    """KPairCap: capacity of each read's final region list = its core regions + one rescue per eligible anchor of the mate (at most 50) + 1."""
    c0 = n0 + min(n1, MAX_RESCUE)
    c1 = n1 + min(c0, MAX_RESCUE)
    return c0 + 1, c1 + 1


class Shapes:
    def __init__(self, o, flat, lens):
        self.F = {f: i for i, f in enumerate(o.LSHAPE_FIELDS)}
        self.I = {f: i for i, f in enumerate(o.LINS_FIELDS)}
        off = np.concatenate([[0], np.cumsum(lens)])
        rows, ins = [], []
        for p in range(len(lens) // 2):
            rd, pi = o.list_shapes(flat[off[2 * p]:off[2 * p + 1]], flat[off[2 * p + 1]:off[2 * p + 2]])
            rows.append(rd)
            ins.append(pi)
        self.rd = np.concatenate(rows)          # one row per read
        self.ins = ins                          # per pair: one row per insertion of mem_matesw
        self.all_ins = np.concatenate(ins) if ins else np.zeros((0, len(self.I)), dtype=np.int64)

    def col(self, name):
        return self.rd[:, self.F[name]]

    def icol(self, name):
        return self.all_ins[:, self.I[name]]

    def count(self, name, value):
        return int((self.col(name) == value).sum())

    def caps(self):
        """per pair: (sum of the two core lists, sum of the two capacities)"""
        n = self.col("regs_out")
        core = n[0::2] + n[1::2]
        cap = np.array([sum(pair_cap(int(a), int(b))) for a, b in zip(n[0::2], n[1::2])], dtype=np.int64)
        return core, cap

    def census(self, chain_min=CHAIN_HEAVY_MIN, dedup_min=DEDUP_HEAVY_MIN, rescue_min=RESCUE_HEAVY_MIN, dedup_heavy=True, classes=False, reads=None):
        """What Batch.heavy_census() must report for these reads (a slice of whole pairs, or all) in ONE run of the batch."""
        sl = slice(None) if reads is None else reads
        occ, regs = self.col("occ")[sl], self.col("regs_in")[sl]
        n = self.col("regs_out")[sl]
        core = n[0::2] + n[1::2]
        cap = np.array([sum(pair_cap(int(a), int(b))) for a, b in zip(n[0::2], n[1::2])], dtype=np.int64)
        hv = (core >= rescue_min) & (cap <= RESCUE_LDS_REGS)
        out = dict(chain_stages=1,
                   chain_short=int(((occ >= chain_min) & (occ <= CHAIN_LDS_SMALL)).sum()),
                   chain_long=int(((occ >= chain_min) & (occ > CHAIN_LDS_SMALL) & (occ <= CHAIN_LDS_OCC)).sum()),
                   dedup=int(((regs >= dedup_min) & (regs <= DEDUP_LDS_REGS)).sum()) if dedup_heavy else 0,
                   rescue=int(hv.sum()))
        out["rescue_170"] = int((hv & (cap <= 170)).sum()) if classes else 0
        out["rescue_340"] = int((hv & (cap > 170) & (cap <= 340)).sum()) if classes else 0
        out["rescue_680"] = int((hv & (cap > 340)).sum()) if classes else int(hv.sum())
        return out

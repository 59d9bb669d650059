"""Generates tests/golden/ext_stage_v1.npz from the reference's own C core (oracle/_ref/libbwaref.so, compiled in place by oracle/Makefile).  Runs only
where the reference's sources exist.

The fixture is DATA: the planted rows of tests/extcases.py's small batches (reads, chain rows, seed rows, frac_rep bits) and the regions the
reference's mem_chain2aln gave for them, read after read, before mem_sort_dedup_patch -- so that tests/test_oracle_golden.py holds the restatement's
ora_chain2aln to the reference where oracle/_ref cannot be built.  (The big batch repeats the main batch's reads and is left out.)

usage: python tests/golden/make_ext_stage_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import extcases  # noqa: E402
import refdrv  # noqa: E402

SIM = os.path.join(os.path.dirname(HERE), "hostsim", "libarx_hostsim.so")


def main():
    c = extcases.build_all()
    fa = c["genome"].write_index(SIM)      # the product's builder writes the reference's index byte for byte (test_index_build.py)
    r = refdrv.Ref(fa)
    out = {"batches": np.array([b.name for b in c["batches"]])}
    for k, b in enumerate(c["batches"]):
        rows = b.rows()
        regs = []
        for rd in b.reads:
            got = r.chain2aln(rd["read"], rd["ch"], rd["sd"], extcases.FRAC_REP_BITS)
            assert got is not None, (b.name, rd["name"])
            regs.append(got)
        out[f"b{k}_seqs"] = rows["seqs"]
        out[f"b{k}_lens"] = rows["lens"]
        out[f"b{k}_n_chain"] = rows["n_chain"]
        out[f"b{k}_n_seed"] = rows["n_seed"]
        out[f"b{k}_chains"] = rows["chains"].astype(np.int32)      # (every value fits: coordinates below 2^18)
        out[f"b{k}_seeds"] = rows["seeds"].astype(np.int32)
        out[f"b{k}_frb"] = rows["frb"]
        out[f"b{k}_reg_off"] = np.concatenate([[0], np.cumsum([len(x) for x in regs])]).astype(np.int32)
        out[f"b{k}_regs"] = np.concatenate(regs).reshape(-1, 20)
    r.close()
    path = os.path.join(HERE, "ext_stage_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

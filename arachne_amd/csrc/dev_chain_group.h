// dev_chain_group.h -- chaining and chain filtering of ONE read by a 16-lane group, four reads per 64-lane wavefront (gfx950 only;
// arx_cold.hip: k_chain_g16; opt-in with ARX_CHAIN_GROUP=1 -- measured no faster than the thread-per-read path, profiles/chain_group/).
//
// 99.7 % of a GRCh38-size batch's reads bring fewer than 64 seed occurrences (median 8).  One thread per read (dev_chain.h, KChain) keeps
// such a read's working set -- B-tree nodes, chain records, seed links, the filter's rank arrays, ~100 B per occurrence -- in per-read
// HBM slices, and mem_chain's loop, the weight walks, the introsort and the filter are chains of dependent loads on them: the kernel waits
// on the latency of a memory system that the co-running seeding kernels keep busy.  Here the group copies the read's occurrences into
// LDS with coalesced loads and the whole working set stays there:
//   * mem_chain's loop and the B-tree (dev_chain.h's chain_build, kbtree semantics unchanged) run in the group's first lane on LDS, with
//     the contigs' ALT flags looked up by the group beforehand (one round trip to memory per read instead of one per chain) and no pass
//     over the read's intervals: frac_rep counts the intervals with more than max_occ (500) occurrences, and KOccFill places 500 of
//     every such interval, so a read with fewer occurrences has none and frac_rep = 0;
//   * the chains' weights (mem_chain_weight): one chain per lane;
//   * ranking (klib's introsort, whose order of equal weights is part of the result) and mem_chain_flt's loop: dev_chain.h's
//     chain_rank_filter in the first lane on LDS (at most 63 chains);
//   * the first lane writes the surviving chains and their seeds to the read's own slices of cout / sout.
// Results are those of chain_and_filter() bit for bit: the same functions run on the same data, only from LDS.
//
// The four groups of a wavefront follow different paths, so nothing here may wait at a workgroup barrier.  A wavefront's LDS accesses
// are performed in the order it issues them; g16_sync() keeps the compiler from moving loads and stores across the hand-offs between
// the lanes of a group.
#pragma once
#include "dev_chain.h"

namespace arx {

__device__ __forceinline__ void g16_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Pools as for chain_and_filter(), all in LDS except cout / sout, for a read with n_occ < OPT_MAX_OCC occurrences; iscr[0, n_occ) holds
// ann_alt of every occurrence's contig on entry.  The 16 lanes of the group call this with the same arguments (group-uniform control flow).
// xch: 4 ints, st: 48 ints (the traversal's stack) of the group's LDS.  Returns (on every lane of the group) the number of chains kept, or
// -1 on pool exhaustion.
__device__ int g16_chain_and_filter(const IndexView &ix, int len, const Seed *occ, const int32_t *occ_rid, int n_occ,
                                    int *next, Chain *ctmp, BtNode *nodes, int cap_nodes, int *iscr, Chain *cout, Seed *sout, int sout_base, int *xch, int *st)
{
	const int sub = threadIdx.x & 15;
	if (len < OPT_MIN_SEED_LEN || n_occ == 0) return 0;
	int *ord = iscr;
	if (sub == 0) {
		BTree bt;
		const int n_ch = chain_build(ix, occ, occ_rid, n_occ, next, ctmp, bt, nodes, cap_nodes, 0.f, iscr); // (iscr is free until the traversal)
		xch[0] = n_ch > 0 ? bt_traverse_st(bt, ord, st) : n_ch; // chains in key order = the array mem_chain returns
	}
	g16_sync();
	const int n = xch[0];
	if (n <= 0) return n;
	for (int i = sub; i < n; i += 16) { Chain &c = ctmp[ord[i]]; c.first = -1; c.kept = 0; c.w = chain_weight(c, occ, next); }
	g16_sync();
	if (sub == 0) {
		chain_rank_filter(n, n_occ, ctmp, occ, iscr);
		xch[1] = chain_emit(n, ord, ctmp, occ, next, cout, sout, sout_base);
	}
	g16_sync();
	return xch[1];
}

} // namespace arx

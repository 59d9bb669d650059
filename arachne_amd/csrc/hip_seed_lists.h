// hip_seed_lists.h -- the list passes of the seeding stage by 16-lane groups: one read per group (a DPP row), four reads per wavefront.
//
// The thread-per-read forms (pipeline.h: KSeedMerge, KOccFill) walk a read's list entry by entry, one dependent round trip to memory each,
// with neighbouring lanes a whole interval slot (CAP_INTV entries, 8 KB) apart.  Here a group takes a read's list in ONE trip -- lane j
// holds entry j -- does the pass in registers with shuffles inside the group, and stores once:
//   k_seed_merge_g16   both interval lists of a read sorted by info: every lane ranks its entry among the group's and stores it at its rank
//   k_occ_fill_g16     a read's intervals expanded into its seed occurrences: the lanes stride over the read's slots, 16 B each, coalesced
// A read whose list is longer than a group (more than 16 entries) is left to the group's first lane, which runs the functor of the
// thread-per-read form on it -- so these kernels compute what those functors compute, and ARX_SEED_LISTS=0 (switches.h), ARX_SW_SIMPLE=1 and
// the host test double keep running the functors themselves.  The two gather passes and the packing of the reads (k_pack_reads) have no
// group form (profiles/seed_lists/README.md says why).
#pragma once
#include <hip/hip_runtime.h>
#include "arx_dev.h"
#include "dev_fm.h"

namespace arx {

constexpr int LIST_GL = 16;             // lanes per read
constexpr int LIST_BLOCK = 256;         // 16 reads per workgroup
struct alignas(16) ListQ { uint64_t a, b; }; // half a Biv, a whole Seed: one 16-byte access (both arrays come from the arena, 256-byte aligned, and hold whole entries)

__device__ __forceinline__ uint64_t list_shfl64(uint64_t v, int src) { return (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, src, LIST_GL) | (uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src, LIST_GL) << 32; }
__device__ __forceinline__ Biv list_load(const Biv *p) { const ListQ *q = (const ListQ *)p; const ListQ lo = q[0], hi = q[1]; Biv b; b.k = lo.a; b.l = lo.b; b.s = hi.a; b.info = hi.b; return b; }
__device__ __forceinline__ void list_store(Biv *p, const Biv &b) { ListQ *q = (ListQ *)p; q[0] = ListQ{b.k, b.l}; q[1] = ListQ{b.s, b.info}; }

// F = KSeedMerge.  n = n_intv[r] + n_strat[r] <= 16: lane j loads entry j (from the read's slot, or from its third-pass list behind it), its
// rank is the number of entries with a smaller info, equal ones by their index -- the order seed_merge()'s insertion sort leaves them in --
// and it stores its entry at its rank.  (Every load of the group is in a register before the first store: the store waits for the
// wavefront's loads.)  The sum of min(s, max_occ) over the group is the read's occurrence count.
template <class F> static __global__ void __launch_bounds__(LIST_BLOCK) k_seed_merge_g16(F f, int n_reads)
{
	const int g = blockIdx.x * LIST_BLOCK + threadIdx.x, r = g / LIST_GL, j = g % LIST_GL; // (n_reads < 2^27: g does not wrap)
	const bool valid = r < n_reads;
	const int n12 = valid ? f.n_intv[r] : 0, n3 = valid ? f.n_strat[r] : 0, n = n12 + n3;
	if (n > LIST_GL) { if (j == 0) f(r, 0); } // the whole group takes this branch or none of it: the shuffles below stay among 16 live lanes
	else {
		Biv *out = f.intv + (size_t)r * CAP_INTV;
		const bool on = j < n;
		Biv e = Biv();
		if (on) e = list_load(j < n12 ? out + j : f.strat + (size_t)r * CAP_STRAT + (j - n12));
		int rank = 0;
#pragma unroll
		for (int i = 0; i < LIST_GL; ++i) {
			const uint64_t ki = list_shfl64(e.info, i);
			rank += i < n && (ki < e.info || (ki == e.info && i < j));
		}
		if (on) list_store(out + rank, e);
		int occ = on ? (e.s > (uint64_t)OPT_MAX_OCC ? OPT_MAX_OCC : (int)e.s) : 0;
#pragma unroll
		for (int d = 1; d < LIST_GL; d <<= 1) occ += __shfl_xor(occ, d, LIST_GL);
		if (valid && j == 0) { f.n_intv[r] = n; f.n_occ[r] = occ; }
	}
}

// F = KOccFill.  n_intv[r] <= 16: lane j holds interval j, its row count min(s, max_occ) and its stride; an inclusive prefix over the group
// gives every interval's slots.  Slot t of the read belongs to the interval i with prefix[i - 1] <= t < prefix[i] (a binary search over
// the lanes, four shuffles), is its row number t - prefix[i - 1], and is written by lane t mod 16: interval by interval, rows ascending,
// as KOccFill writes them.
template <class F> static __global__ void __launch_bounds__(LIST_BLOCK) k_occ_fill_g16(F f, int n_reads)
{
	const int g = blockIdx.x * LIST_BLOCK + threadIdx.x, r = g / LIST_GL, j = g % LIST_GL;
	const bool valid = r < n_reads;
	const int n = valid ? f.n_intv[r] : 0;
	if (n > LIST_GL) { if (j == 0) f(r, 0); }
	else {
		Biv p = Biv();
		if (j < n) p = list_load(f.intv + (size_t)r * CAP_INTV + j);
		const bool capped = p.s > (uint64_t)OPT_MAX_OCC;
		const int cnt = j < n ? (capped ? OPT_MAX_OCC : (int)p.s) : 0;
		const uint64_t step = capped ? p.s / OPT_MAX_OCC : 1;
		int incl = cnt;
#pragma unroll
		for (int d = 1; d < LIST_GL; d <<= 1) { const int v = __shfl_up(incl, d, LIST_GL); if (j >= d) incl += v; }
		const int total = __shfl(incl, LIST_GL - 1, LIST_GL); // (a whole number of rounds for the group: the shuffles in the loop find 16 live lanes)
		ListQ *dst = (ListQ *)(f.occ_seed + (valid ? f.occ_off[r] : 0));
		for (int t0 = 0; t0 < total; t0 += LIST_GL) {
			const int t = t0 + j;
			int i = 0; // the number of intervals that end at or before slot t
#pragma unroll
			for (int h = LIST_GL / 2; h >= 1; h >>= 1) { const int v = __shfl(incl, i + h - 1, LIST_GL); if (v <= t) i += h; }
			const int first = __shfl(incl - cnt, i, LIST_GL);
			const uint64_t k = list_shfl64(p.k, i), st = list_shfl64(step, i), info = list_shfl64(p.info, i);
			if (t < total) {
				const uint32_t qbeg = (uint32_t)(info >> 32), len = (uint32_t)info - qbeg;
				dst[t] = ListQ{k + (uint64_t)(t - first) * st, (uint64_t)qbeg | (uint64_t)len << 32}; // Seed{rbeg, qbeg, len}
			}
		}
	}
}

} // namespace arx

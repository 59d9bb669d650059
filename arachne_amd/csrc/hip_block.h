// hip_block.h -- workgroup-cooperative primitives for kernels that give one work item (a barcode) to a whole 1024-lane
// workgroup: strided parallel-for with barrier, block scan, bitonic key/value sort, arg-max.  The device logic written
// against this handle (dev_rfa.h) keeps its control flow uniform over the workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace arx {

#ifndef ARX_BLOCK_LANES
#define ARX_BLOCK_LANES 1024 // 6.4 ms (256) -> 4.3 (512) -> 3.8 (1024) per 350 k-pair batch: a barcode is one workgroup and the kernel is latency-bound
#endif
constexpr int BLOCK_LANES = ARX_BLOCK_LANES, SORT_LDS = 4096;
// A barcode of TELLseq size (tens of pairs) does not need 1024 lanes and 60 KB of LDS: small barcodes run in workgroups of
// SMALL_LANES lanes with a SMALL_SORT-entry sort buffer (15 KB: ten workgroups per CU instead of two).
constexpr int SMALL_LANES = 256, SMALL_SORT = 1024;
// Largest P that sort_kv orders by counting ranks instead of by the bitonic network, per class (at most the class's lanes: one entry per lane).
// 0: never.  The rank sort has 2 barrier phases against the network's 38 at P = 256, but P * P comparisons against 36 * P / 2, and the network's
// stages run in LDS at about 0.3 us each: per 4,096 sorts of 1,024-lane workgroups 0.32 / 0.68 / 1.89 ms by rank against 0.14 / 0.20 / 0.28 ms
// by the network at P = 256 / 512 / 1,024, and 0.024 / 0.046 / 0.103 against 0.023 / 0.028 / 0.038 ms at P = 64 / 128 / 256 in the 256-lane class
// (profiles/rfa_sweeps/README.md).  It loses at every size, so it stays behind ARX_BLOCK_RANK_SORT (switches.h), which overrides both constants.
constexpr int RANK_SORT_MAX = 0, SMALL_RANK_SORT_MAX = 0;

template <int BLOCK_LANES, int SORT_LDS> struct HipBlockT {
	int tid;
	uint64_t *l64; // BLOCK_LANES words of LDS
	int32_t *l32;  // BLOCK_LANES + 1 words of LDS

	template <class F> __device__ __forceinline__ void pfor(int n, F f)
	{
		for (int i = tid; i < n; i += BLOCK_LANES) f(i);
		__syncthreads();
	}
	template <class F> __device__ __forceinline__ void single(F f)
	{
		if (tid == 0) f();
		__syncthreads();
	}
	// out[i] = sum of in[0..i), i in [0, n]; returns the total.  Every lane scans one contiguous chunk.
	__device__ int exclusive_scan(const int32_t *in, int32_t *out, int n)
	{
		const int per = (n + BLOCK_LANES - 1) / BLOCK_LANES, b = tid * per, e = b + per < n ? b + per : n;
		int sum = 0;
		for (int i = b; i < e; ++i) sum += in[i];
		l32[tid] = sum;
		__syncthreads();
		if (tid < 64) { // one wave scans the partial sums, BLOCK_LANES / 64 per lane
			constexpr int PER = BLOCK_LANES / 64;
			int a[PER], t = 0;
#pragma unroll
			for (int x = 0; x < PER; ++x) { a[x] = l32[PER * tid + x]; t += a[x]; }
			int incl = t;
			for (int d = 1; d < 64; d <<= 1) { int o = __shfl_up(incl, d, 64); if (tid >= d) incl += o; }
			int ex = incl - t;
#pragma unroll
			for (int x = 0; x < PER; ++x) { l32[PER * tid + x] = ex; ex += a[x]; }
			if (tid == 63) l32[BLOCK_LANES] = incl;
		}
		__syncthreads();
		int run = l32[tid];
		const int total = l32[BLOCK_LANES];
		for (int i = b; i < e; ++i) { const int x = in[i]; out[i] = run; run += x; }
		if (tid == 0) out[n] = total;
		__syncthreads();
		return total;
	}
	// ascending sort of P = 2^k (key, value) pairs by (key, (uint32)value): by rank for P <= rank_max, else the bitonic network, which sorts
	// up to SORT_LDS pairs in LDS.  Entries equal in both words are interchangeable, so the two forms write the same arrays.
	uint64_t *sk; int32_t *sv; // SORT_LDS entries of LDS each
	int rank_max;              // <= BLOCK_LANES (launch_block clamps it)
	__device__ void sort_kv(uint64_t *k, int32_t *v, int P)
	{
		if (P <= rank_max) { sort_kv_rank(k, v, P); return; }
		if (P <= SORT_LDS) {
			for (int t = tid; t < P; t += BLOCK_LANES) { sk[t] = k[t]; sv[t] = v[t]; }
			__syncthreads();
			sort_kv_in(sk, sv, P);
			for (int t = tid; t < P; t += BLOCK_LANES) { k[t] = sk[t]; v[t] = sv[t]; }
			__syncthreads();
		} else sort_kv_in(k, v, P);
	}
	// One entry per lane: its place is the number of entries that are smaller, or equal and in front of it (so entries that occur several times,
	// the (~0, -1) padding among them, get places of their own).  Every lane reads the same LDS word at a time -- a broadcast, no bank conflict --
	// and writes its entry once: two barrier phases instead of one per stage of the network.
	__device__ void sort_kv_rank(uint64_t *k, int32_t *v, int P)
	{
		typedef __attribute__((address_space(3))) uint64_t lds_u64; // sk / sv are generic pointers: say that they point into LDS
		typedef __attribute__((address_space(3))) int32_t lds_i32;
		const lds_u64 *lk = (const lds_u64 *)sk; const lds_i32 *lv = (const lds_i32 *)sv;
		uint64_t mk = 0; uint32_t mv = 0;
		if (tid < P) { mk = k[tid]; mv = (uint32_t)v[tid]; sk[tid] = mk; sv[tid] = (int32_t)mv; }
		__syncthreads(); // every lane has read its entry of k / v: they may be overwritten
		if (tid < P) {
			// Eight entries per round, all sixteen reads issued before the first comparison, and the comparison without a branch (| and &, not ||
			// and &&): written with short-circuit operators every entry costs two LDS latencies one after the other, three times the network's time
			constexpr int U = 8;
			unsigned rank = 0;
			for (int j0 = 0; j0 < P; j0 += U) {
				uint64_t kj[U]; uint32_t vj[U];
#pragma unroll
				for (int u = 0; u < U; ++u) { const int j = j0 + u < P ? j0 + u : P - 1; kj[u] = lk[j]; vj[u] = (uint32_t)lv[j]; } // (P < U: the last entry again, not counted)
#pragma unroll
				for (int u = 0; u < U; ++u) {
					const int j = j0 + u;
					const unsigned before = (unsigned)(kj[u] < mk) | ((unsigned)(kj[u] == mk) & ((unsigned)(vj[u] < mv) | ((unsigned)(vj[u] == mv) & (unsigned)(j < tid))));
					rank += before & (unsigned)(j < P);
				}
			}
			k[rank] = mk; v[rank] = (int32_t)mv; // rank < P: the entry itself is not counted
		}
		__syncthreads();
	}
	__device__ void sort_kv_in(uint64_t *k, int32_t *v, int P)
	{
		for (int size = 2; size <= P; size <<= 1)
			for (int stride = size >> 1; stride > 0; stride >>= 1) {
				for (int t = tid; t < (P >> 1); t += BLOCK_LANES) {
					const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), hi = lo | stride;
					const bool up = (lo & size) == 0;
					const uint64_t ka = k[lo], kb = k[hi];
					const uint32_t va = (uint32_t)v[lo], vb = (uint32_t)v[hi];
					const bool gt = ka > kb || (ka == kb && va > vb);
					if (gt == up) { k[lo] = kb; k[hi] = ka; v[lo] = (int32_t)vb; v[hi] = (int32_t)va; }
				}
				__syncthreads();
			}
	}
	// largest key over i in [0, n) (0 = none), ties to the smallest i; every lane gets the result
	template <class F> __device__ void argmax(int n, F keyf, uint64_t *key, int *idx)
	{
		uint64_t bk = 0; int bi = 0x7fffffff;
		for (int i = tid; i < n; i += BLOCK_LANES) { const uint64_t x = keyf(i); if (x > bk) { bk = x; bi = i; } } // i ascends: the first maximum stays
		for (int d = 32; d > 0; d >>= 1) {
			const uint64_t ok = (uint64_t)__shfl_xor((unsigned long long)bk, d, 64); const int oi = __shfl_xor(bi, d, 64);
			if (ok > bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
		}
		if ((tid & 63) == 0) { l64[tid >> 6] = bk; l32[tid >> 6] = bi; }
		__syncthreads();
		bk = l64[0]; bi = l32[0];
		for (int w = 1; w < BLOCK_LANES / 64; ++w) { const uint64_t ok = l64[w]; const int oi = l32[w]; if (ok > bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; } }
		__syncthreads(); // the LDS words are reused by the next call
		*key = bk; *idx = bi;
	}
};

using HipBlock = HipBlockT<BLOCK_LANES, SORT_LDS>;

// cls / want: only the items whose class byte equals `want` (cls == nullptr: all)
template <class F, int LANES, int SORT> __global__ __launch_bounds__(LANES) void k_block_items(F f, int n, const uint8_t *cls, int want, int rank_max)
{
	__shared__ uint64_t l64[LANES];
	__shared__ int32_t l32[LANES + 1];
	__shared__ uint64_t sk[SORT];
	__shared__ int32_t sv[SORT];
	HipBlockT<LANES, SORT> blk{(int)threadIdx.x, l64, l32, sk, sv, rank_max < LANES ? rank_max : LANES};
	for (int b = blockIdx.x; b < n; b += gridDim.x) {
		if (cls && cls[b] != want) continue; // uniform over the workgroup
		f(b, blk);
		__syncthreads();
	}
}

} // namespace arx

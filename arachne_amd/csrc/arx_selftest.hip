// arx_selftest.hip -- the self-test entries of the three DP kernel families (include/arachne_amd.h: arx_selftest_extend,
// arx_selftest_rescue_sw, arx_selftest_gen_cigar) and of the records phase's decimal text (arx_selftest_rec_text).  They take plain host arrays, build what the pipeline would hand the kernels (an IndexView
// with only the packed text set, class-binned extension tasks, rescue tasks with their mates, staged CIGAR regions) and launch the production
// code through HipRT, so that tests/test_dp_kernels_gpu.py can compare every output field with ksw_extend2 / ksw_align2 / ksw_global2.
// arx_selftest_block runs the workgroup primitives of hip_block.h (scan, bitonic sort, arg-max) through k_block_items itself, one case per workgroup, and
// arx_selftest_rfa (selftest_rfa.h) the whole placement stage on alignments the caller made up (tests/test_block_primitives_gpu.py, tests/test_rfa_cases_gpu.py).
// arx_selftest_reg2aln (selftest_reg2aln.h) runs stage 6 itself -- Pipeline::stage_reg2aln with its slot loop, k_reg2aln_nw_g16 per band class, the launch
// that takes what they hand on, the one-thread path and compact() -- on regions the caller made up (tests/test_cigar_stage_gpu.py).
// arx_selftest_post (selftest_post.h) runs PostStage::run -- the CIGAR walk, the duplicate table, the split pass -- on candidates the caller made up
// (tests/test_post_stage_gpu.py).
// arx_selftest_ext_stage (selftest_ext.h) runs stage 4 itself -- Pipeline::stage_extend with its chain state machines, the round loop, run_extend,
// the gather and the de-duplication -- on chains and seeds the caller made up (tests/test_ext_stage_gpu.py).
// Its own unit so that the unit of the list-bookkeeping kernels does not grow.
#include <climits>
#include <vector>
#include "../../include/arachne_amd.h"
#include "hip_rt.h"
#include "pipeline.h"
#include "dev_records_full.h"
#include "selftest_rfa.h"
#include "selftest_reg2aln.h"
#include "selftest_post.h"
#include "selftest_ext.h"

namespace arx {

// the target (and query) of a region staged the way k_reg2aln_nw_g16 stages them, then bwa_gen_cigar2 by the class kernel's tilings
template <int LO, int HI>
static __global__ void __launch_bounds__(64) k_selftest_gen_cigar(const uint8_t *q, const int32_t *q_off, const int32_t *qlen, const uint8_t *t,
                                                                  const int32_t *t_off, const int32_t *tlen, const int32_t *w, const int32_t *cap,
                                                                  int cig_w, uint8_t *z, const int64_t *z_off, int n, int32_t *out, uint32_t *cig)
{
	__shared__ uint8_t lds_q[4][NW_Q_CAP];
	__shared__ uint8_t lds_t[4][NW_T_CAP];
	__shared__ __attribute__((aligned(16))) uint8_t lds_z[4][NW_ZL_BYTES];
	const int grp = threadIdx.x >> 4, l = threadIdx.x & 15;
	for (int i = blockIdx.x * 4 + grp; i < n; i += gridDim.x * 4) {
		NwSeg sg; sg.q = lds_q[grp]; sg.t = lds_t[grp]; sg.qlen = qlen[i]; sg.tlen = tlen[i];
		for (int k = l; k < sg.qlen; k += 16) lds_q[grp][k] = q[q_off[i] + k];
		for (int k = l; k < sg.tlen; k += 16) lds_t[grp][k] = t[t_off[i] + k];
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		int score = 0, n_cigar = 0, NM = -1;
		const bool done = gen_cigar2_g16<LO, HI>(sg, w[i], z + z_off[i], lds_z[grp], cig + (size_t)i * cig_w, cap[i], &score, &n_cigar, &NM);
		if (l == 0) { out[4 * i] = done ? score : 0; out[4 * i + 1] = done ? n_cigar : 0; out[4 * i + 2] = done ? NM : -1; out[4 * i + 3] = done ? 0 : 1; }
		__builtin_amdgcn_wave_barrier(); // the LDS rows are reused by the group's next region
	}
}

// the records phase's decimal text (dev_records_full.h), one input per lane, written character by character as the fill asks for it
struct KSelftestRecText {
	const int32_t *a, *b; int kind; uint8_t *out; int32_t *len;
	ARX_DEV void operator()(int i, int) const
	{
		uint8_t *o = out + 32 * (size_t)i;
		int l;
		if (kind == 0) { l = int_len(a[i]); for (int k = 0; k < l; ++k) o[k] = (uint8_t)int_char(a[i], k); }
		else { const uint64_t t = dm_scaled_signed(a[i], b[i]); l = dm_len(a[i], t); for (int k = 0; k < l; ++k) o[k] = (uint8_t)dm_char(a[i] < 0, t, k); }
		for (int k = l; k < 32; ++k) o[k] = 0;
		len[i] = l;
	}
};

// one case per workgroup of hip_block.h's primitives, started by HipRT::launch_block like the placement kernel (k_block_items<F, LANES, SORT>: the
// production LDS layout and launch bounds).  A value every lane receives is read back from lanes 0, 63, 64 and LANES - 1 (slots 0..3).
struct KSelftestBlock {
	const int32_t *op, *n; const int64_t *in_off, *out_off; const uint64_t *keys; const int32_t *vals; uint64_t *ok; int32_t *ov;
	template <int L> static __device__ int slot_of(int tid) { return tid == 0 ? 0 : tid == 63 ? 1 : tid == 64 ? 2 : tid == L - 1 ? 3 : -1; }
	template <int L, int S> __device__ void operator()(int c, HipBlockT<L, S> &blk) const
	{
		const int m = n[c], slot = slot_of<L>(blk.tid);
		const uint64_t *k = keys + in_off[c]; const int32_t *v = vals + in_off[c];
		uint64_t *o64 = ok + out_off[c]; int32_t *o32 = ov + out_off[c];
		if (op[c] == ARX_BLOCK_OP_SCAN) { // o32[0..m] = the scan, o32[m + 1 + slot] = the return value in four lanes
			const int total = blk.exclusive_scan(v, o32, m);
			if (slot >= 0) o32[m + 1 + slot] = total;
		} else if (op[c] == ARX_BLOCK_OP_SORT) { // in place on the output arrays, as rfa_barcode sorts its scratch
			blk.pfor(m, [&](int i) { o64[i] = k[i]; o32[i] = v[i]; });
			blk.sort_kv(o64, o32, m);
		} else {
			uint64_t bk; int bi;
			blk.argmax(m, [&](int i) -> uint64_t { return k[i]; }, &bk, &bi);
			if (slot >= 0) { o64[slot] = bk; o32[slot] = bi; }
		}
	}
};

static bool one_strand(int64_t a, int64_t b, int64_t l_pac) // both ends inside the same strand of [0, 2 * l_pac)
{
	if (a < 0 || b < 0 || a >= 2 * l_pac || b >= 2 * l_pac) return false;
	return (a < l_pac) == (b < l_pac);
}

static IndexView pac_view(HipRT &rt, const uint8_t *pac, int64_t l_pac)
{
	IndexView ix = IndexView();
	const size_t bytes = (size_t)((l_pac + 3) / 4);
	uint8_t *d = rt.alloc<uint8_t>(bytes);
	rt.h2d(d, pac, bytes);
	ix.pac = d; ix.l_pac = l_pac;
	return ix;
}

} // namespace arx

extern "C" int arx_selftest_extend(int32_t device, const uint8_t *pac, int64_t l_pac, const uint8_t *bases, int64_t n_bases, int32_t n, const int64_t *task8,
                                   int32_t mode, int32_t grid_cap, int32_t *res6)
{
	using namespace arx;
	if (n < 0 || mode < 0 || mode > 3 || l_pac < 1 || n_bases < 0 || n_bases > INT_MAX || (n > 0 && (!pac || !bases || !task8 || !res6))) return ARX_E_ARG;
	std::vector<ExtTask> tk((size_t)EXT_CLASSES * (n + 1));
	int32_t n_class[EXT_CLASSES] = {0};
	for (int i = 0; i < n; ++i) {
		const int64_t *r = task8 + 8 * (size_t)i;
		const int64_t tpos = r[0], qoff = r[1], qlen = r[2], tlen = r[3], qdir = r[4], tdir = r[5], w = r[6], h0 = r[7];
		if (qlen < 1 || qlen > MAX_READ_LEN || (qdir != 1 && qdir != -1) || (tdir != 1 && tdir != -1)) return ARX_E_ARG;
		const int64_t qlast = qoff + (qlen - 1) * qdir;
		if (qoff < 0 || qoff >= n_bases || qlast < 0 || qlast >= n_bases) return ARX_E_ARG;
		if (tlen < 0 || tlen > 2 * l_pac || (tlen > 0 && !one_strand(tpos, tpos + (tlen - 1) * tdir, l_pac))) return ARX_E_ARG; // tlen == 0: a window that ends at the seed (a contig's edge)
		if (w < 1 || w > INT_MAX || h0 < 1 || h0 > MAX_READ_LEN * OPT_A) return ARX_E_ARG;
		ExtTask t;
		t.tpos = tpos; t.owner = i; t.qoff = (int32_t)qoff; t.qlen = (int32_t)qlen; t.tlen = (int32_t)tlen;
		t.qdir = (int32_t)qdir; t.tdir = (int32_t)tdir; t.w = (int32_t)w; t.h0 = (int32_t)h0;
		const int c = ext_class(t.qlen);
		tk[(size_t)c * (n + 1) + n_class[c]++] = t; // stride-spaced class slots, as pipeline.h's stage_extend bins them
	}
	if (n == 0) return ARX_OK;
	try {
		HipRT rt;
		if (!rt.init(device).empty()) return ARX_E_DEVICE;
		rt.timing = false;
		rt.sw.ext_merge_below = mode == 1 ? INT_MAX : 0;
		rt.sw.ext_old = mode == 2;
		rt.sw.sw_simple = mode == 3;
		if (grid_cap > 0) { rt.n_cu = 1; rt.sw.coop_bpc = grid_cap; rt.sw.bpc = grid_cap; } // (the one-thread form: max_blocks() = grid_cap)
		KExtend f{pac_view(rt, pac, l_pac), rt.alloc<uint8_t>((size_t)n_bases + 1), rt.alloc<ExtTask>(tk.size()), rt.alloc<ExtRes>((size_t)n)};
		rt.h2d((void *)f.bases, bases, (size_t)n_bases);
		rt.h2d((void *)f.tasks, tk.data(), tk.size() * sizeof(ExtTask));
		rt.memset_bytes(f.res, 0x80, (size_t)n * sizeof(ExtRes)); // a task that is never run shows up as a mismatch
		rt.run_extend("selftest_extend", n_class, n + 1, f);
		ARX_HIP_CHECK(hipStreamSynchronize(rt.stream));
		static_assert(sizeof(ExtRes) == 6 * sizeof(int32_t), "ExtRes is six int32");
		rt.d2h(res6, f.res, (size_t)n * sizeof(ExtRes));
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
	return ARX_OK;
}

extern "C" int arx_selftest_rescue_sw(int32_t device, const uint8_t *pac, int64_t l_pac, const uint8_t *mates, int64_t n_bases, int32_t n, const int32_t *mate_off,
                                      const int32_t *mate_len, const int64_t *win2, int32_t max_len, int32_t filter, int32_t sw_simple, int32_t grid_cap, int32_t *res7)
{
	using namespace arx;
	if (n < 0 || l_pac < 1 || n_bases < 0 || n_bases > INT_MAX || max_len < 1 || max_len > MAX_READ_LEN) return ARX_E_ARG;
	if (n > 0 && (!pac || !mates || !mate_off || !mate_len || !win2 || !res7)) return ARX_E_ARG;
	std::vector<SwTask> tk((size_t)n);
	for (int i = 0; i < n; ++i) {
		const int64_t rb = win2[2 * (size_t)i], re = win2[2 * (size_t)i + 1];
		if (mate_len[i] < 1 || mate_len[i] > max_len || mate_off[i] < 0 || (int64_t)mate_off[i] + mate_len[i] > n_bases) return ARX_E_ARG;
		if (re - rb < 1 || re - rb > SW_T_CAP || !one_strand(rb, re - 1, l_pac)) return ARX_E_ARG;
		SwTask t;
		t.rb = rb; t.re = re; t.pair = i >> 1; t.o = i & 1; t.slot = i; t.pad = 0; // read 2 * pair + o is mate i
		tk[i] = t;
	}
	if (n == 0) return ARX_OK;
	try {
		HipRT rt;
		if (!rt.init(device).empty()) return ARX_E_DEVICE;
		rt.timing = false;
		rt.sw.sw_filter = filter ? 1 : 0;
		rt.sw.sw_filter_stats = 0;
		rt.sw.sw_simple = sw_simple != 0;
		if (grid_cap > 0) { rt.n_cu = 1; rt.sw.coop_bpc = grid_cap; rt.sw.bpc = grid_cap; }
		// the one-thread form keeps its mate, window and row maxima in per-slot scratch: one slot per thread of its grid
		const int q_cap = (max_len + 15) & ~15, t_cap = SW_T_CAP;
		const int slots = ((n + 63) / 64 < rt.max_blocks() ? (n + 63) / 64 : rt.max_blocks()) * 64;
		KSwU8 f{pac_view(rt, pac, l_pac), rt.alloc<uint8_t>((size_t)n_bases + 1), rt.alloc<int32_t>((size_t)n), rt.alloc<int32_t>((size_t)n),
		        rt.alloc<SwTask>((size_t)n), rt.alloc<U8Res>((size_t)n), rt.sw.sw_simple ? rt.alloc<uint8_t>((size_t)slots * (q_cap + 2 * t_cap)) : nullptr, q_cap, t_cap};
		rt.h2d((void *)f.bases, mates, (size_t)n_bases);
		rt.h2d((void *)f.base_off, mate_off, (size_t)n * 4);
		rt.h2d((void *)f.lens, mate_len, (size_t)n * 4);
		rt.h2d((void *)f.tasks, tk.data(), tk.size() * sizeof(SwTask));
		rt.memset_bytes(f.res, 0x80, (size_t)n * sizeof(U8Res));
		rt.run_sw_u8("selftest_sw_u8", n, f, max_len);
		ARX_HIP_CHECK(hipStreamSynchronize(rt.stream));
		static_assert(sizeof(U8Res) == 7 * sizeof(int32_t), "U8Res is seven int32");
		rt.d2h(res7, f.res, (size_t)n * sizeof(U8Res));
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
	return ARX_OK;
}

extern "C" int arx_selftest_gen_cigar(int32_t device, int32_t n, const uint8_t *q, const int32_t *q_off, const int32_t *qlen, const uint8_t *t, const int32_t *t_off,
                                      const int32_t *tlen, const int32_t *w, const int32_t *cap, int32_t cig_w, int32_t klass, int32_t *out4, uint32_t *cigar)
{
	using namespace arx;
	static const int HI[6] = {2, 4, 8, 16, 16, 16}; // columns per lane of the widest tiling each kernel holds: rows of 16 * HI bytes of traceback matrix
	if (n < 0 || klass < 0 || klass > 5 || cig_w < 1) return ARX_E_ARG;
	if (n > 0 && (!q || !q_off || !qlen || !t || !t_off || !tlen || !w || !cap || !out4 || !cigar)) return ARX_E_ARG;
	std::vector<int64_t> z_off((size_t)n + 1, 0);
	int64_t nq = 0, nt = 0;
	for (int i = 0; i < n; ++i) {
		if (qlen[i] < 1 || qlen[i] > NW_Q_CAP || tlen[i] < 1 || tlen[i] > NW_T_CAP || w[i] < 0 || cap[i] < 1 || cap[i] > cig_w) return ARX_E_ARG;
		if (q_off[i] < 0 || t_off[i] < 0) return ARX_E_ARG;
		nq = nq > (int64_t)q_off[i] + qlen[i] ? nq : (int64_t)q_off[i] + qlen[i];
		nt = nt > (int64_t)t_off[i] + tlen[i] ? nt : (int64_t)t_off[i] + tlen[i];
		z_off[i + 1] = z_off[i] + (((int64_t)tlen[i] * 16 * HI[klass] + 63) & ~(int64_t)63);
	}
	if (n == 0) return ARX_OK;
	try {
		HipRT rt;
		if (!rt.init(device).empty()) return ARX_E_DEVICE;
		uint8_t *dq = rt.alloc<uint8_t>((size_t)nq), *dt = rt.alloc<uint8_t>((size_t)nt), *dz = rt.alloc<uint8_t>((size_t)z_off[n] + 64);
		int32_t *di = rt.alloc<int32_t>((size_t)n * 6), *dout = rt.alloc<int32_t>((size_t)n * 4);
		int64_t *dzo = rt.alloc<int64_t>((size_t)n);
		uint32_t *dcig = rt.alloc<uint32_t>((size_t)n * cig_w);
		rt.h2d(dq, q, (size_t)nq); rt.h2d(dt, t, (size_t)nt);
		const int32_t *src[6] = {q_off, qlen, t_off, tlen, w, cap};
		for (int k = 0; k < 6; ++k) rt.h2d(di + (size_t)k * n, src[k], (size_t)n * 4);
		rt.h2d(dzo, z_off.data(), (size_t)n * 8);
		rt.memset_bytes(dout, 0x80, (size_t)n * 16);
		rt.memset0(dcig, (size_t)n * cig_w * 4);
		const int blocks = (n + 3) / 4 < rt.n_cu * 4 ? (n + 3) / 4 : rt.n_cu * 4;
		// the instantiations of HipRT::run_reg2aln_nw: its five class kernels and the one that holds every tiling
		using Kernel = decltype(&k_selftest_gen_cigar<1, 2>);
		static constexpr Kernel by_class[6] = {k_selftest_gen_cigar<1, 2>, k_selftest_gen_cigar<2, 4>, k_selftest_gen_cigar<4, 8>, k_selftest_gen_cigar<8, 16>,
		                                       k_selftest_gen_cigar<16, 16>, k_selftest_gen_cigar<1, 16>};
		rt.start("k_selftest_gen_cigar", by_class[klass], dim3(blocks), dim3(64), 0, dq, di, di + n, dt, di + 2 * (size_t)n, di + 3 * (size_t)n, di + 4 * (size_t)n,
		         di + 5 * (size_t)n, cig_w, dz, dzo, n, dout, dcig);
		ARX_HIP_CHECK(hipStreamSynchronize(rt.stream));
		rt.d2h(out4, dout, (size_t)n * 16);
		rt.d2h(cigar, dcig, (size_t)n * cig_w * 4);
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
	return ARX_OK;
}

extern "C" int arx_selftest_rec_text(int32_t device, int32_t n, const int32_t *a, const int32_t *b, int32_t kind, uint8_t *out, int32_t *len)
{
	using namespace arx;
	if (n < 0 || kind < 0 || kind > 1 || (n > 0 && (!a || !out || !len || (kind == 1 && !b)))) return ARX_E_ARG;
	if (kind == 1) for (int i = 0; i < n; ++i) if (b[i] <= 0) return ARX_E_ARG;
	if (n == 0) return ARX_OK;
	try {
		HipRT rt;
		if (!rt.init(device).empty()) return ARX_E_DEVICE;
		rt.timing = false;
		int32_t *da = rt.alloc<int32_t>((size_t)n), *db = rt.alloc<int32_t>((size_t)n), *dl = rt.alloc<int32_t>((size_t)n);
		uint8_t *dout = rt.alloc<uint8_t>(32 * (size_t)n);
		rt.h2d(da, a, 4 * (size_t)n);
		if (kind == 1) rt.h2d(db, b, 4 * (size_t)n);
		KSelftestRecText f{da, db, kind, dout, dl};
		rt.launch_wide("selftest_rec_text", n, f);
		ARX_HIP_CHECK(hipStreamSynchronize(rt.stream));
		rt.d2h(out, dout, 32 * (size_t)n);
		rt.d2h(len, dl, 4 * (size_t)n);
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
	return ARX_OK;
}

extern "C" int arx_selftest_block_shape(int32_t klass, int32_t *lanes, int32_t *sort_entries)
{
	if (klass < 0 || klass > 1 || !lanes || !sort_entries) return ARX_E_ARG;
	*lanes = klass == 0 ? arx::BLOCK_LANES : arx::SMALL_LANES;
	*sort_entries = klass == 0 ? arx::SORT_LDS : arx::SMALL_SORT;
	return ARX_OK;
}

extern "C" int arx_selftest_block(int32_t device, int32_t klass, int32_t n_cases, const int32_t *op, const int32_t *n, const int64_t *in_off, const int64_t *out_off,
                                  const uint64_t *keys, const int32_t *vals, int64_t n_in, uint64_t *out_keys, int32_t *out_vals, int64_t n_out)
{
	using namespace arx;
	if (n_cases < 0 || klass < 0 || klass > 1 || n_in < 0 || n_out < 0) return ARX_E_ARG;
	if (n_cases > 0 && (!op || !n || !in_off || !out_off || !out_keys || !out_vals || (n_in > 0 && (!keys || !vals)))) return ARX_E_ARG;
	for (int c = 0; c < n_cases; ++c) { // every index a workgroup forms lies inside the arrays
		if (n[c] < 0 || n[c] > (1 << 24) || in_off[c] < 0 || out_off[c] < 0 || in_off[c] + n[c] > n_in) return ARX_E_ARG;
		int64_t need;
		if (op[c] == ARX_BLOCK_OP_SCAN) need = (int64_t)n[c] + 5;
		else if (op[c] == ARX_BLOCK_OP_SORT) { need = n[c]; if (n[c] < 1 || (n[c] & (n[c] - 1))) return ARX_E_ARG; }
		else if (op[c] == ARX_BLOCK_OP_ARGMAX) need = 4;
		else return ARX_E_ARG;
		if (out_off[c] + need > n_out) return ARX_E_ARG;
	}
	if (n_cases == 0) return ARX_OK;
	try {
		HipRT rt;
		if (!rt.init(device).empty()) return ARX_E_DEVICE;
		rt.timing = false;
		int32_t *d_i = rt.alloc<int32_t>(2 * (size_t)n_cases), *d_v = rt.alloc<int32_t>((size_t)n_in + 1), *d_ov = rt.alloc<int32_t>((size_t)n_out + 1);
		int64_t *d_o = rt.alloc<int64_t>(2 * (size_t)n_cases);
		uint64_t *d_k = rt.alloc<uint64_t>((size_t)n_in + 1), *d_ok = rt.alloc<uint64_t>((size_t)n_out + 1);
		rt.h2d(d_i, op, 4 * (size_t)n_cases); rt.h2d(d_i + n_cases, n, 4 * (size_t)n_cases);
		rt.h2d(d_o, in_off, 8 * (size_t)n_cases); rt.h2d(d_o + n_cases, out_off, 8 * (size_t)n_cases);
		rt.h2d(d_k, keys, 8 * (size_t)n_in); rt.h2d(d_v, vals, 4 * (size_t)n_in);
		rt.h2d(d_ok, out_keys, 8 * (size_t)n_out); rt.h2d(d_ov, out_vals, 4 * (size_t)n_out); // what no case writes comes back as the caller filled it
		KSelftestBlock f{d_i, d_i + n_cases, d_o, d_o + n_cases, d_k, d_v, d_ok, d_ov};
		const std::vector<uint8_t> small((size_t)n_cases, 1);
		rt.launch_block("selftest_block", n_cases, f, klass == 1 ? small.data() : nullptr);
		ARX_HIP_CHECK(hipStreamSynchronize(rt.stream));
		rt.d2h(out_keys, d_ok, 8 * (size_t)n_out);
		rt.d2h(out_vals, d_ov, 4 * (size_t)n_out);
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
	return ARX_OK;
}

extern "C" int arx_selftest_rfa(int32_t device, int32_t n_reads, const int64_t *reg_off, const int64_t *regs, const int64_t *alns, const uint32_t *cigars, int64_t n_cig,
                                const int32_t *lens, int32_t n_barcodes, const int64_t *bc_pair_off, const uint8_t *do_rfa, int32_t penalty, int64_t l_pac,
                                const int64_t *ann_off, int32_t n_seqs, const int64_t *cen_start, const int64_t *cen_end, int32_t rfa_small, double mapq_guard,
                                int32_t *cand_off, void *cands, int64_t cand_cap, void *bc_out, uint8_t *cls, int64_t *n_host_mapq)
{
	using namespace arx;
	try {
		HipRT rt;
		if (!rt.init(device).empty()) return ARX_E_DEVICE;
		rt.timing = false;
		return selftest_rfa_run(rt, n_reads, reg_off, regs, alns, cigars, n_cig, lens, n_barcodes, bc_pair_off, do_rfa, penalty, l_pac, ann_off, n_seqs, cen_start, cen_end,
		                        rfa_small, mapq_guard, cand_off, cands, cand_cap, bc_out, cls, n_host_mapq);
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
}

// The bins of the backward sweeps as the forward kernels fill them: Pipeline::stage_seed itself on the caller's reads, with the runtime's
// record of the bins switched on (hip_rt.h seed_bins_record)
extern "C" int arx_selftest_seed_bins(arx_ctx *ctx, const uint8_t *bases, const int32_t *lens, int32_t n_reads, int32_t *n_launches, int32_t *rec, int32_t rec_cap,
                                      int32_t *task_n, int64_t task_cap, int32_t *bin_ids, int64_t bin_cap)
{
	using namespace arx;
	const IndexView *ix = ctx_index_view(ctx);
	if (!ix || !bases || !lens || n_reads < 1 || !n_launches || !rec || !task_n || !bin_ids || rec_cap < 0 || task_cap < 0 || bin_cap < 0) return ARX_E_ARG;
	int64_t tot = 0;
	for (int i = 0; i < n_reads; ++i) { if (lens[i] < 0 || lens[i] > MAX_READ_LEN) return ARX_E_ARG; tot += lens[i]; }
	if (tot >= ((int64_t)1 << 31) - 64) return ARX_E_TOO_LARGE;
	*n_launches = 0;
	try {
		HipRT rt;
		if (!rt.init(arx_ctx_device(ctx)).empty()) return ARX_E_DEVICE;
		rt.timing = false;
		rt.seed_bins_log_on = true;
		Pipeline<HipRT> pipe(rt, *ix);
		Pipeline<HipRT>::DeviceBatch db = pipe.upload(bases, lens, n_reads);
		Pipeline<HipRT>::Work w;
		int rc = ARX_OK;
		try { if (pipe.stage_seed(db, w) == -2) rc = ARX_E_TOO_LARGE; rt.sync(); } catch (...) { pipe.release(db); throw; }
		pipe.release(db);
		if (rc != ARX_OK) return rc;
		int64_t nt = 0, nb = 0;
		for (const HipRT::SeedBinsRecord &r : rt.seed_bins_log) {
			if (*n_launches >= rec_cap || nt + r.n > task_cap || nb + r.cnt[0] + r.cnt[1] + r.cnt[2] + r.cnt[3] > bin_cap) return ARX_E_TOO_LARGE;
			int32_t *o = rec + 8 * (size_t)*n_launches;
			o[0] = r.t0; o[1] = r.n; for (int c = 0; c < 4; ++c) o[2 + c] = r.cnt[c]; o[6] = (int32_t)r.err; o[7] = 0;
			for (int32_t v : r.task_n) task_n[nt++] = v;
			for (int c = 0; c < 4; ++c) for (int32_t v : r.bin[c]) bin_ids[nb++] = v;
			++*n_launches;
		}
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
	return ARX_OK;
}

// Stage 6 on the caller's regions: Pipeline::stage_reg2aln on a runtime of its own, with ctx's index and the ARX_* switches as they are at the call
extern "C" int arx_selftest_reg2aln(arx_ctx *ctx, const uint8_t *bases, const int32_t *lens, int32_t n_reads, const int32_t *cap, const int32_t *n_regs, const int64_t *regs,
                                    int32_t *reg_off, void *alns, int64_t aln_cap, uint32_t *cigars, int64_t cig_cap, int64_t *n_cig, uint32_t *err, int64_t *census,
                                    int64_t census_cap, int32_t grid_cap)
{
	using namespace arx;
	const IndexView *ix = ctx_index_view(ctx);
	if (!ix) return ARX_E_ARG;
	try {
		HipRT rt;
		if (!rt.init(arx_ctx_device(ctx)).empty()) return ARX_E_DEVICE;
		rt.timing = false;
		if (grid_cap > 0) { rt.n_cu = 1; rt.sw.coop_bpc = grid_cap; } // class launches of at most grid_cap workgroups, two for what they hand on: every group takes many regions
		return selftest_reg2aln_run(rt, *ix, bases, lens, n_reads, cap, n_regs, regs, reg_off, alns, aln_cap, cigars, cig_cap, n_cig, err, census, census_cap);
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
}

// The passes between placement and the BAM records on the caller's candidates: PostStage::run on a runtime of its own, with ctx's index and the ARX_*
// switches as they are at the call.  (order: the host double's item order; a GPU's arrival order is not ours to choose)
extern "C" int arx_selftest_post(arx_ctx *ctx, int32_t n_reads, const int64_t *cand_off, const int64_t *cands, int64_t n_regs, const int64_t *regs, const int64_t *alns,
                                 const uint32_t *cigars, int64_t n_cig, const uint8_t *bases, const int32_t *lens, int32_t n_barcodes, const int64_t *bc_pair_off,
                                 int32_t penalty, const int64_t *cen_start, const int64_t *cen_end, void *post, void *split, int32_t *mm_ref, int32_t *mm_read,
                                 int64_t mm_cap, int64_t *n_mm, int32_t *table, int64_t table_cap, int32_t *n_table, int32_t *home, int32_t grid_cap, int32_t)
{
	using namespace arx;
	const IndexView *ix = ctx_index_view(ctx);
	if (!ix) return ARX_E_ARG;
	try {
		HipRT rt;
		if (!rt.init(arx_ctx_device(ctx)).empty()) return ARX_E_DEVICE;
		rt.timing = false;
		if (grid_cap > 0) { rt.n_cu = 1; rt.sw.bpc = grid_cap; rt.sw.wide = false; } // launch_wide's capped form on grid_cap workgroups: every lane strides through many items
		return selftest_post_run(rt, *ix, n_reads, cand_off, cands, n_regs, regs, alns, cigars, n_cig, bases, lens, n_barcodes, bc_pair_off, penalty, cen_start, cen_end,
		                         post, split, mm_ref, mm_read, mm_cap, n_mm, table, table_cap, n_table, home);
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
}

// Stage 4 on the caller's chains: Pipeline::stage_extend on a runtime of its own, with ctx's index and the ARX_* switches as they are at the call.
// (order: the host double's item order; a GPU's arrival order is not ours to choose)
extern "C" int arx_selftest_ext_stage(arx_ctx *ctx, const uint8_t *bases, const int32_t *lens, int32_t n_reads, const int32_t *n_chain, const int64_t *chains, const int32_t *n_seed,
                                      const int64_t *seeds, const uint32_t *frac_rep_bits, int32_t *ext_off, int64_t *ext_regs, int32_t *core_off, int64_t *core_regs,
                                      int64_t reg_cap, int32_t *core_clean, int64_t *stats, int32_t *rounds, int64_t rounds_cap, int32_t *done_round, int32_t *chain_n_regs,
                                      uint32_t *err, int32_t grid_cap, int32_t)
{
	using namespace arx;
	const IndexView *ix = ctx_index_view(ctx);
	if (!ix) return ARX_E_ARG;
	try {
		HipRT rt;
		if (!rt.init(arx_ctx_device(ctx)).empty()) return ARX_E_DEVICE;
		rt.timing = false;
		if (grid_cap > 0) { rt.n_cu = 1; rt.sw.bpc = grid_cap; rt.sw.coop_bpc = grid_cap; rt.sw.wide = false; } // every launch of the stage on grid_cap workgroups: every lane strides through many items
		return selftest_ext_run(rt, *ix, bases, lens, n_reads, n_chain, chains, n_seed, seeds, frac_rep_bits, ext_off, ext_regs, core_off, core_regs, reg_cap, core_clean, stats,
		                        rounds, rounds_cap, done_round, chain_n_regs, err);
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
}

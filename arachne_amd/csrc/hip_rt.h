// hip_rt.h -- the HIP runtime policy of Pipeline<RT>: device memory, kernel launches on one stream (every one through start(), i.e.
// hip_launch.h's checked primitive), device scan, per-kernel timing with HIP events.  gfx950 only.  What the runtime holds for itself -- its
// streams, events, arena slabs, staging and scratch -- are owners of hip_res.h; palloc / pfree stay raw: they are the interface the host double mirrors.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <map>
#include <string>
#include <vector>
#include <stdexcept>
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <climits>
#include "hip_res.h"
#include "hip_sw_coop.h"
#include "hip_block.h"
#include "hip_nw_coop.h"
#include "hip_fm_coop.h"
#include "hip_seed_lists.h"
#include "index_build.h"
#include "switches.h"

struct arx_ctx; // include/arachne_amd.h

namespace arx {

// generic grid-stride launchers; slot = global thread index (always < max_slots) selects per-thread scratch
#ifndef ARX_ITEMS_WPE
#define ARX_ITEMS_WPE 1 // (experiments) wavefronts per SIMD the thread-per-item kernels are compiled for
#endif
// per-functor register budget (wavefronts per SIMD the kernel is compiled for); specialised where a measurement says so
template <class F> struct ItemsWpe { static constexpr int v = ARX_ITEMS_WPE; };
template <class F> __global__ void __launch_bounds__(64, ItemsWpe<F>::v) k_items(F f, int n)
{
	const int slot = blockIdx.x * blockDim.x + threadIdx.x;
	const long long step = (long long)gridDim.x * blockDim.x; // i + step must not wrap: launches of more than 2^30 items exist (arx_open: ARX_SA_DENSE=4 at GRCh38 size)
	for (long long i = slot; i < n; i += step) f((int)i, slot);
}
// DP kernels: each thread owns words [threadIdx.x + j*blockDim.x] of the block's LDS, i.e. a [column][lane] layout
template <class F> __global__ void __launch_bounds__(64) k_rows(F f, int n)
{
	extern __shared__ uint32_t lds_rows[];
	const int slot = blockIdx.x * blockDim.x + threadIdx.x;
	const long long step = (long long)gridDim.x * blockDim.x;
	for (long long i = slot; i < n; i += step) f((int)i, slot, lds_rows + threadIdx.x, (int)blockDim.x);
}

struct CastI64 { __host__ __device__ int64_t operator()(const int32_t &x) const { return (int64_t)x; } };

struct KernelTimer { double ms = 0; int64_t calls = 0, items = 0; };

std::string product_bwt_sa(const uint8_t *pac, size_t pac_bytes, int64_t l_pac, const uint64_t cnt_fwd[4], const std::string &prefix); // arx_index.hip
const IndexView *ctx_index_view(::arx_ctx *ctx); // arx_api.hip: the device-resident index of an open context (null: no context); for the self-test entries that need one

struct HipRT {
	BatchSwitches sw; // the ARX_* environment as it was when this runtime (= its batch handle, context or device feeder) was created (switches.h)
	static const char *name() { return "hip:gfx950"; }
	static BwtSaFn bwt_sa_fn() { return product_bwt_sa; } // arx_index_build: the suffix sort runs in HBM
	Stream own_stream;      // declared before everything that is used on it: it is the last to go, and waits for what is on it
	hipStream_t stream = 0; // the stream of the next launch: own_stream, or the side stream inside on_aux
	// side streams for launches that keep a few wavefronts busy (the heavy-item kernels, the above-cap reads' chaining walk, one CIGAR band
	// class): they run beside the launches that follow on the main stream until aux_join().  Several forks may precede one join: a side
	// stream runs its forks in order and the join waits for the last of each.  There are two (`lane`), for the one stage with three launches
	// side by side (the split chaining); every other fork is on the first.  A part whose switch is off (aux_on) runs f on the main stream.
	// Lifetime rule: everything a side-stream launch touches is arena memory of the current stage, and aux_join() runs before the stage
	// returns, before any arena_rewind and before any host read-back of what the launch wrote.
	static constexpr int AUX_LANES = 2;
	Stream aux[AUX_LANES]; Event ev_fork, ev_join[AUX_LANES]; bool aux_pending[AUX_LANES] = {false, false};
	bool aux_on(AuxPart p) const { return sw.aux_stream && (p == AUX_CHAIN ? sw.aux_chain : p == AUX_DEDUP ? sw.aux_dedup : p == AUX_NW ? sw.aux_nw : sw.aux_rescue); }
	template <class L> void on_aux(AuxPart part, L f, int lane = 0)
	{
		if (!aux_on(part)) { f(); return; }
		if (!ev_fork) ev_fork.create(hipEventDisableTiming);
		if (!aux[lane]) { aux[lane].create(); ev_join[lane].create(hipEventDisableTiming); }
		ARX_HIP_CHECK(hipEventRecord(ev_fork, stream)); ARX_HIP_CHECK(hipStreamWaitEvent(aux[lane], ev_fork, 0));
		hipStream_t main_stream = stream;
		stream = aux[lane];
		try { f(); } catch (...) { stream = main_stream; throw; } // (a launch that fails in f must not leave the runtime on the side stream)
		stream = main_stream;
		ARX_HIP_CHECK(hipEventRecord(ev_join[lane], aux[lane]));
		aux_pending[lane] = true;
	}
	void aux_join()
	{
		for (int l = 0; l < AUX_LANES; ++l) if (aux_pending[l]) { ARX_HIP_CHECK(hipStreamWaitEvent(stream, ev_join[l], 0)); aux_pending[l] = false; }
	}
	// one scope, two launches over the same n items with whatever `between` starts (forks with scopes of their own) in between: a pass that
	// classifies the items and the launch that takes what the pass left
	template <class FC, class FL, class B> void launch_classified(const char *nm, int n, const FC &classify, const FL &rest, B between)
	{
		if (n <= 0) return;
		Scope sc(*this, nm, n);
		items_kernel(nm, n, classify, INT_MAX);
		between();
		items_kernel(nm, n, rest, sw.wide ? INT_MAX : max_blocks());
	}
	// every launch of the runtime: on the current stream (the side stream inside on_aux), checked at once under its name (hip_launch.h)
	template <class... P> void start(const LaunchName &name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, typename as_declared<P>::type... args) { hip_launch(name, kernel, grid, block, lds_bytes, stream, args...); }
	// a kernel's opt-in to `bytes` of dynamic LDS.  It applies to the device that is current when it is made, so it is made once per runtime (=
	// per device context), not once per process.  Every caller asks for its kernel's largest footprint, a constant: a kernel is remembered by
	// its address alone and a second call for it does nothing, whatever `bytes` it names
	std::vector<const void *> lds_opted_in;
	template <class K> void allow_dynamic_lds(K kernel, size_t bytes)
	{
		for (const void *k : lds_opted_in) if (k == (const void *)kernel) return;
		ARX_HIP_CHECK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
		lds_opted_in.push_back((const void *)kernel);
	}
	int n_cu = 256;
	bool timing = false;
	std::map<std::string, KernelTimer> tm;
	DevScratch scan_tmp; DevBuf d_total; PinnedBuf pinned;

	int dev = 0;
	void bind() { (void)hipSetDevice(dev); }           // the current device is per host thread
	void set_timing(bool on) { timing = on; }
	std::string init(int device)
	{
		int n = 0;
		dev = device;
		if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return "no HIP device visible: libarachne_amd.so needs an MI355X (there is no CPU fallback)";
		if (device < 0 || device >= n) return "device index out of range";
		if (hipSetDevice(device) != hipSuccess) return "hipSetDevice failed";
		hipDeviceProp_t p;
		if (hipGetDeviceProperties(&p, device) != hipSuccess) return "hipGetDeviceProperties failed";
		n_cu = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
		try { own_stream.create(); stream = own_stream; } catch (const HipError &) { return "hipStreamCreate failed"; }
		try { d_total.alloc(8); } catch (const HipError &) { return "hipMalloc failed"; }
		try { pinned.alloc(64); } catch (const HipError &) { return "hipHostMalloc failed"; }
		return "";
	}
	~HipRT()
	{
		if (sw.sw_filter_stats && sw_tasks_seen) fprintf(stderr, "[arx] rescue alignments queued %lld, run after the pre-filter %lld\n", (long long)sw_tasks_seen, (long long)sw_tasks_run);
	}
	// Work memory of a batch comes from a per-runtime arena: slabs obtained once with hipMalloc, bump-allocated, handed back
	// only by rewinding to a mark or resetting the whole (there is no free of a single block).  Steady state therefore has
	// no hipMalloc/hipFree at all -- both synchronise the device and would serialise the batches that run on other streams.
	struct Slab { DevBuf mem; size_t used; };
	std::vector<Slab> slabs;
	template <class T> T *alloc(size_t n)
	{
		size_t bytes = ((n ? n : 1) * sizeof(T) + 255) & ~(size_t)255;
		for (auto &sl : slabs) if (sl.mem.bytes - sl.used >= bytes) { char *r = sl.mem.as<char>() + sl.used; sl.used += bytes; return (T *)r; }
		slabs.push_back(Slab{DevBuf(bytes > ((size_t)1 << 30) ? bytes : ((size_t)1 << 30)), bytes});
		return slabs.back().mem.as<T>();
	}
	void arena_reset() { for (auto &sl : slabs) sl.used = 0; }
	std::vector<size_t> arena_mark() const { std::vector<size_t> m; for (auto &sl : slabs) m.push_back(sl.used); return m; }
	void arena_rewind(const std::vector<size_t> &m) { for (size_t i = 0; i < slabs.size(); ++i) slabs[i].used = i < m.size() ? m[i] : 0; }
	// persistent memory.  Raw hipMalloc / hipFree on purpose: the pair is the runtime interface (SimRT has the same), what it returns is its caller's to free
	template <class T> T *palloc(size_t n) { void *p = 0; ARX_HIP_CHECK(hipMalloc(&p, (n ? n : 1) * sizeof(T))); return (T *)p; }
	void pfree(void *p) { if (p) (void)hipFree(p); }
	void h2d(void *d, const void *s, size_t bytes) { if (bytes) { ARX_HIP_CHECK(hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, stream)); ARX_HIP_CHECK(hipStreamSynchronize(stream)); } }
	void d2h(void *d, const void *s, size_t bytes)
	{
		if (!bytes) return;
		if (bytes <= 64 && pinned.p) { // small read-backs (round counters, error word, scan totals) go through pinned memory
			ARX_HIP_CHECK(hipMemcpyAsync(pinned.p, s, bytes, hipMemcpyDeviceToHost, stream));
			ARX_HIP_CHECK(hipStreamSynchronize(stream));
			memcpy(d, pinned.p, bytes);
			return;
		}
		ARX_HIP_CHECK(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToHost, stream));
		ARX_HIP_CHECK(hipStreamSynchronize(stream));
	}
	void d2h_async(void *d, const void *s, size_t bytes) { if (bytes) ARX_HIP_CHECK(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToHost, stream)); } // sync() before the data is read
	// staging for uploads: pinned host memory owned by the runtime, grown on demand.  stage() waits for the copies of the previous
	// use (the stream has long passed them when a batch is reset after its results were fetched); h2d_staged() only enqueues.
	PinnedBuf stage_buf;
	void *stage(size_t bytes)
	{
		ARX_HIP_CHECK(hipStreamSynchronize(stream));
		if (bytes > stage_buf.bytes) stage_buf.alloc(bytes + bytes / 8 + 4096);
		return stage_buf.p;
	}
	void h2d_staged(void *d, const void *staged, size_t bytes) { if (bytes) ARX_HIP_CHECK(hipMemcpyAsync(d, staged, bytes, hipMemcpyHostToDevice, stream)); }
	// Host memory the caller has page-locked (arx_host_register): copies to and from it are DMA at PCIe speed without a staging copy --
	// hipMemcpyAsync finds that out by itself for the results (d2h); an upload from it skips the runtime's own pinned staging buffer.
	static int host_register(void *p, size_t bytes) { const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable); if (e != hipSuccess) (void)hipGetLastError(); return e == hipSuccess ? 0 : -1; }
	static int host_unregister(void *p) { const hipError_t e = hipHostUnregister(p); if (e != hipSuccess) (void)hipGetLastError(); return e == hipSuccess ? 0 : -1; }
	static bool host_pinned(const void *p)
	{
		hipPointerAttribute_t a;
		if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
		return a.type == hipMemoryTypeHost;
	}
	void h2d_pinned(void *d, const void *s, size_t bytes) // from page-locked caller memory; returns when the copy is done (the caller may reuse the array)
	{
		if (!bytes) return;
		ARX_HIP_CHECK(hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, stream));
		ARX_HIP_CHECK(hipStreamSynchronize(stream));
	}
	uint64_t free_bytes() const { size_t f = 0, t = 0; return hipMemGetInfo(&f, &t) == hipSuccess ? (uint64_t)f : 0; }
	void d2d(void *d, const void *s, size_t bytes) { if (bytes) ARX_HIP_CHECK(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, stream)); }
	void memset0(void *d, size_t bytes) { ARX_HIP_CHECK(hipMemsetAsync(d, 0, bytes, stream)); }
	void memset_bytes(void *d, int v, size_t bytes) { ARX_HIP_CHECK(hipMemsetAsync(d, v, bytes, stream)); }
	void sync() { ARX_HIP_CHECK(hipStreamSynchronize(stream)); }

	// launch shapes (sw.bpc, sw.coop_bpc, ...: switches.h)
	int max_blocks() const { return n_cu * sw.bpc; }
	int coop_blocks(int n) const { int b = (n + 3) / 4, cap = n_cu * sw.coop_bpc; return b < cap ? b : cap; }
	int max_slots() const { return max_blocks() * 64; }
	int max_slots_small() const { return n_cu * 64; }
	// seeding kernels: 4 * ARX_SEED_WPE resident blocks per CU (their register budget is compiled for that many waves per SIMD)
	int seed_bpc() const { return sw.seed_bpc.value_or(4 * ARX_SEED_WPE); }
	int strat_bpc() const { return sw.strat_bpc.value_or(4 * ARX_SEED_WPE); } // the third seeding pass
	int max_seed_slots() const { return n_cu * seed_bpc() * 64; }
	int seed_row = SEED_ROW;                                   // LDS bytes per lane for its read
	void set_seed_read_len(int max_len) { seed_row = seed_row_bytes(max_len); }
	// the batch's reads as nibble rows of seed_row bytes (hip_fm_coop.h: k_pack_reads): what the seeding kernels stage into LDS
	const uint32_t *seed_qn = nullptr;
	void seed_prepare(const uint8_t *bases, const int32_t *base_off, const int32_t *lens, int n_reads)
	{
		seed_bins = SeedBins(); // (arena memory of the batch before)
		if (sw.sw_simple || n_reads <= 0) return;
		const int rw = seed_row >> 2;
		uint32_t *q = alloc<uint32_t>((size_t)n_reads * rw + 8);
		Scope sc(*this, "seed_pack", n_reads);
		const long long total = (long long)n_reads * rw;
		start("k_pack_reads", k_pack_reads, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, bases, base_off, lens, n_reads, rw, q);
		seed_qn = q;
	}
	// the list passes of the seeding stage, one read per 16-lane group (hip_seed_lists.h); f is the functor of the thread-per-read form, which
	// the group's first lane runs on a read with more than 16 entries and every launch runs under ARX_SEED_LISTS=0 or ARX_SW_SIMPLE
	static dim3 list_grid(int n_reads) { return dim3((unsigned)(((long long)n_reads * LIST_GL + LIST_BLOCK - 1) / LIST_BLOCK)); }
	bool seed_lists_ok() const { return sw.seed_lists && !sw.sw_simple; }
	template <class F> void run_seed_merge(const char *nm, int n, const F &f)
	{
		if (n <= 0) return;
		Scope sc(*this, nm, n);
		start({"k_seed_merge_g16", nm}, k_seed_merge_g16<F>, list_grid(n), dim3(LIST_BLOCK), 0, f, n);
	}
	template <class F> void run_occ_fill(const char *nm, int n, const F &f)
	{
		if (n <= 0) return;
		Scope sc(*this, nm, n);
		start({"k_occ_fill_g16", nm}, k_occ_fill_g16<F>, list_grid(n), dim3(LIST_BLOCK), 0, f, n);
	}

	// Kernel timing: a pair of HIP events around each launch on the launch stream, recorded without blocking and
	// resolved (hipEventElapsedTime) the next time the stream is known to be idle.
	struct Pending { Event a, b; const char *nm; int64_t items; };
	std::vector<Pending> pending;
	std::vector<Event> free_events;
	Event get_event()
	{
		if (free_events.empty()) return Event(hipEventDefault);
		Event e = std::move(free_events.back()); free_events.pop_back(); return e;
	}
	struct Scope {
		HipRT &rt; Pending p; bool on; const char *tn;
		Scope(HipRT &r, const char *n, int64_t it) : rt(r), on(r.timing), tn(r.sw.trace_launches ? n : nullptr)
		{
			if (tn) { fprintf(stderr, "[arx launch] %s (%lld items) ...\n", tn, (long long)it); fflush(stderr); }
			if (!on) return;
			p.a = rt.get_event(); p.b = rt.get_event(); p.nm = n; p.items = it;
			(void)hipEventRecord(p.a, rt.stream);
		}
		~Scope()
		{
			if (on) { (void)hipEventRecord(p.b, rt.stream); rt.pending.push_back(std::move(p)); }
			if (tn) { (void)hipStreamSynchronize(rt.stream); fprintf(stderr, "[arx launch] %s done\n", tn); fflush(stderr); }
		}
	};
	void resolve_timers()
	{
		if (pending.empty()) return;
		(void)hipStreamSynchronize(stream);
		static FILE *launch_log = sw_open_launch_log(); // diagnostics: one line per launch; one file per process (switches.h)
		for (auto &p : pending) {
			float ms = 0;
			(void)hipEventElapsedTime(&ms, p.a, p.b);
			if (launch_log) fprintf(launch_log, "%s\t%lld\t%.4f\n", p.nm, (long long)p.items, ms);
			KernelTimer &t = tm[p.nm]; t.ms += ms; ++t.calls; t.items += p.items;
			free_events.push_back(std::move(p.a)); free_events.push_back(std::move(p.b));
		}
		pending.clear();
		if (launch_log) fflush(launch_log);
	}
	std::map<std::string, KernelTimer> &timers() { resolve_timers(); return tm; }
	void timers_reset(bool enable) { resolve_timers(); tm.clear(); timing = enable; }

	// The thread-per-item launches: functor f over n items with k_items<F>, on (n + 63) / 64 blocks of 64 lanes or on `cap` of them
	// grid-striding, whichever is fewer.  items_kernel() is the launch alone, for a caller that has a Scope open.
	template <class F> void items_kernel(const char *nm, int n, const F &f, int cap)
	{
		const int blocks = (n + 63) / 64;
		start({"k_items", nm}, k_items<F>, dim3(blocks < cap ? blocks : cap), dim3(64), 0, f, n);
	}
	template <class F> void launch_items(const char *nm, int n, const F &f, int cap)
	{
		if (n <= 0) return;
		Scope sc(*this, nm, n);
		items_kernel(nm, n, f, cap);
	}
	template <class F> void launch(const char *nm, int n, const F &f) { launch_items(nm, n, f, max_blocks()); }
	// for functors that use no per-slot scratch: one item per lane, as many blocks as that takes -- the hardware hands blocks to CUs
	// as they free up, which balances kernels whose items differ a lot in cost better than a fixed grid-stride assignment
	template <class F> void launch_wide(const char *nm, int n, const F &f) { launch_items(nm, n, f, sw.wide ? INT_MAX : max_blocks()); }
	template <class F> void launch_small(const char *nm, int n, const F &f) { launch_items(nm, n, f, n_cu); }
	// "cold" kernels (list bookkeeping: dedup, rescue_step) are instantiated in arx_cold.hip, a translation unit of its own (-O3 like
	// the rest since round 2; arx_dev.h ks_introsort has the story of the -O1 build they needed before)
	template <class F> void launch_cold(const char *nm, int n, const F &f);
	// ks_introsort's budget flag (arx_dev.h) of both device translation units into a batch's error word; no host round trip of its own
	void merge_sort_fail(uint32_t *err) { start("k_merge_sort_fail", k_merge_sort_fail, dim3(1), dim3(1), 0, err); merge_sort_fail_cold(err); }
	void merge_sort_fail_cold(uint32_t *err); // arx_cold.hip
	// rescue replay of the pairs with long lists, lists staged in LDS (arx_cold.hip)
	bool rescue_heavy_ok() const { return sw.rescue_heavy; }
	template <class F> void run_rescue_heavy(const char *nm, int n, const int32_t *list, const F &f);
	// chaining of the reads with many seed occurrences, one wavefront per read on a working set in LDS (arx_cold.hip); f.heavy_list / f.n_heavy
	bool chain_heavy_ok() const { return sw.chain_heavy; }
	template <class F> void run_chain_heavy(const char *nm, int n_reads, const F &f);
	// opt-in (ARX_CHAIN_GROUP=1): chaining of the reads below the heavy kernel's threshold, one 16-lane group per read on a working set in LDS
	// (arx_cold.hip: k_chain_g16; f.grp_max, f.mid_list / f.n_mid)
	bool chain_group_ok() const { return sw.chain_group; }
	template <class F> void run_chain_group(const char *nm, int n_reads, const F &f);
	bool dedup_heavy_ok() const { return sw.dedup_heavy; }
	template <class F> void run_dedup_heavy(const char *nm, int n_reads, const F &f); // likewise the region lists of such reads (f.eh_words ints of scratch per workgroup)
	// the de-duplication with its heavy reads listed by a pass of their own (KDedupList), then k_dedup_heavy on the side stream beside the
	// thread-per-read launch; false (nothing launched) where the side stream's dedup part is off.  The caller joins
	template <class F> bool run_dedup_forked(const char *nm, const char *nm_heavy, int n_reads, const F &f);
	template <class F> void launch_cold_impl(const char *nm, int n, const F &f, bool wide = false) { launch_items(nm, n, f, wide && sw.wide ? INT_MAX : max_blocks()); }
	// one work item per BLOCK_LANES-lane workgroup (hip_block.h); f(item, HipBlock&)
	// small (host, may be null): small[i] = 1 sends item i to a SMALL_LANES-lane workgroup
	template <class F> void launch_block(const char *nm, int n, const F &f, const uint8_t *small = nullptr)
	{
		if (n <= 0) return;
		Scope sc(*this, nm, n);
		int n_small = 0;
		if (small) for (int i = 0; i < n; ++i) n_small += small[i] ? 1 : 0;
		const int rank = sw.block_rank_sort.value_or(RANK_SORT_MAX), rank_small = sw.block_rank_sort.value_or(SMALL_RANK_SORT_MAX); // the kernel keeps them within its lanes
		if (n_small == 0) {
			int blocks = n < n_cu * 8 ? n : n_cu * 8;
			start({"k_block_items<BLOCK_LANES>", nm}, k_block_items<F, BLOCK_LANES, SORT_LDS>, dim3(blocks), dim3(BLOCK_LANES), 0, f, n, nullptr, 0, rank);
		} else {
			uint8_t *d = alloc<uint8_t>((size_t)n + 8);
			h2d(d, small, (size_t)n);
			int blocks = n_small < n_cu * 32 ? n_small : n_cu * 32;
			start({"k_block_items<SMALL_LANES>", nm}, k_block_items<F, SMALL_LANES, SMALL_SORT>, dim3(blocks), dim3(SMALL_LANES), 0, f, n, d, 1, rank_small);
			if (n_small < n) {
				blocks = n - n_small < n_cu * 8 ? n - n_small : n_cu * 8;
				start({"k_block_items<BLOCK_LANES>", nm}, k_block_items<F, BLOCK_LANES, SORT_LDS>, dim3(blocks), dim3(BLOCK_LANES), 0, f, n, d, 0, rank);
			}
		}
	}
	// rescue SW: 16 lanes per alignment (hip_sw_coop.h); sw.sw_simple selects the one-thread-per-alignment kernel for A/B runs
	template <class F> void run_sw_u8(const char *nm, int n, const F &f, int max_len)
	{
		if (n <= 0) return;
		if (sw.sw_simple) { launch_rows(nm, n, f, 16 * ((max_len + 15) / 16)); return; }
		const int blocks = coop_blocks(n);
		int32_t *order = nullptr, *n_order = nullptr;
		if (sw.sw_filter) { // tasks that provably stay below min_seed_len never reach the DP (dev_sw.h: sw_prefilter_serial)
			order = alloc<int32_t>((size_t)n + 1); n_order = order + n;
			memset0(n_order, 4);
			Scope sc(*this, "sw_filter", n);
			start("k_sw_filter_g16", k_sw_filter_g16, dim3(blocks), dim3(64), 0, f.ix, f.bases, f.base_off, f.lens, f.tasks, f.res, n, order, n_order);
		}
		{
			Scope sc(*this, nm, n);
			// <32>: mates of 250+ bases: ksw_i16's eight stripes of up to 32 cells; shorter mates of the same batch take the byte form inside
			const auto kern = max_len <= 160 ? k_sw_u8_g16<10> : max_len * OPT_A < 250 ? k_sw_u8_g16<16> : k_sw_u8_g16<32>;
			start({"k_sw_u8_g16", nm, max_len <= 160 ? 10 : max_len * OPT_A < 250 ? 16 : 32}, kern, dim3(blocks), dim3(64), 0, f.ix, f.bases, f.base_off, f.lens, f.tasks, f.res, n, order, n_order);
		}
		if (sw.sw_filter_stats) { int32_t k = 0; d2h(&k, n_order, 4); sw_tasks_seen += n; sw_tasks_run += k; }
	}
	int64_t sw_tasks_seen = 0, sw_tasks_run = 0;
	// seeding: persistent lanes, items handed out in chunks (hip_fm_coop.h); f is one of pipeline.h's KSeedFwd1 / KSeedFwd2 / KSeedBwd,
	// f.scratch holds max_slots() forward lists
	// diagnostics (ARX_SEED_STATS=1): lane utilisation of the persistent-lane seeding kernels, printed per launch
	DevBuf seed_dbg_buf;
	unsigned long long *seed_dbg()
	{
		if (!sw.seed_stats) return nullptr;
		if (!seed_dbg_buf.p) seed_dbg_buf.alloc(32);
		memset0(seed_dbg_buf.p, 32);
		return seed_dbg_buf.as<unsigned long long>();
	}
	void seed_dbg_report(const char *nm, int n)
	{
		if (!seed_dbg_buf.p) return; // (only seed_dbg() allocates it: sw.seed_stats is on)
		unsigned long long h[4];
		d2h(h, seed_dbg_buf.p, 32);
		fprintf(stderr, "[arx seed stats] %s: %d items, %llu waves, %.0f iterations/wave, %.1f lanes extending per iteration, %.0f slow-path entries/wave\n", nm, n, h[3],
		        h[3] ? (double)h[0] / h[3] : 0.0, h[0] ? (double)h[1] / h[0] : 0.0, h[3] ? (double)h[2] / h[3] : 0.0);
	}
	// opt-in census of the backward sweeps (arx_batch_debug_seed_census; tests assert from it which kernel took which task).  Everything it
	// reports is in device memory after a launch anyway -- the bins' sizes (cnt[0..3]), the hand-off list's length (heavy[n]), the per-task flags
	// (1: handed to k_seed_bwd_wave, 2: left to KSeedBwdTail) -- so switched on it copies them home after the launch and adds them up; switched
	// off (the default) it is one untaken branch on the host: no round trip, no kernel argument.
	// [0] backward launches, [1..4] tasks in the 16 / 21 / 32 / 64-lane bins, [5] tasks flagged for k_seed_bwd_wave, [6] tasks flagged for the
	// tail, [7] length of the hand-off lists k_seed_bwd_wave was given
	bool seed_census_on = false;
	int64_t seed_census[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	void seed_census_add(int n, const int32_t *cnt, const int32_t *n_heavy, const uint8_t *flag)
	{
		if (!seed_census_on) return;
		++seed_census[0];
		if (cnt) { int32_t h[4]; d2h(h, cnt, 16); for (int c = 0; c < 4; ++c) seed_census[1 + c] += h[c]; }
		if (n_heavy) { int32_t nh = 0; d2h(&nh, n_heavy, 4); seed_census[7] += nh; }
		if (flag) {
			std::vector<uint8_t> fl((size_t)n);
			d2h(fl.data(), flag, (size_t)n);
			for (uint8_t f : fl) { seed_census[5] += f == 1; seed_census[6] += f == 2; }
		}
	}
	// opt-in census of the heavy-item lists (arx_batch_debug_heavy_census; tests assert from it which items the wavefront-per-item kernels of
	// arx_cold.hip took).  The lists and their lengths are in device memory after the launches that fill them anyway, so switched on it copies
	// them home and counts; switched off (the default) it is one untaken branch on the host per stage: no round trip, no kernel argument, no
	// counter inside a kernel.
	// [0] chaining stages, [1] reads listed for k_chain_heavy with up to CHAIN_LDS_SMALL occurrences (its short launch), [2] with more (its long
	// launch), [3] reads listed for k_dedup_heavy, [4] pairs listed for k_rescue_heavy, [5..7] those pairs by the LDS class of their two
	// capacities together (up to 170 / 340 / RESCUE_LDS_REGS records) when the replay is launched per class, otherwise all in [7]
	bool heavy_census_on = false;
	int64_t heavy_census[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	void heavy_census_chain(int n_reads, const int32_t *list, const int32_t *n_heavy, const int32_t *occ_off, int split)
	{
		if (!heavy_census_on) return;
		++heavy_census[0];
		int32_t nh = 0;
		if (!list) return;
		d2h(&nh, n_heavy, 4);
		if (nh <= 0) return;
		std::vector<int32_t> l((size_t)nh), off((size_t)n_reads + 1);
		d2h(l.data(), list, 4 * (size_t)nh);
		d2h(off.data(), occ_off, 4 * ((size_t)n_reads + 1));
		for (int32_t r : l) ++heavy_census[off[(size_t)r + 1] - off[(size_t)r] <= split ? 1 : 2];
	}
	void heavy_census_dedup(const int32_t *n_heavy)
	{
		if (!heavy_census_on || !n_heavy) return;
		int32_t nh = 0;
		d2h(&nh, n_heavy, 4);
		heavy_census[3] += nh;
	}
	void heavy_census_rescue(int n_reads, int n_heavy, const int32_t *list, const int32_t *preg_off)
	{
		if (!heavy_census_on || n_heavy <= 0) return;
		heavy_census[4] += n_heavy;
		if (!sw.rescue_lds_classes) { heavy_census[7] += n_heavy; return; }
		std::vector<int32_t> l((size_t)n_heavy), off((size_t)n_reads + 1);
		d2h(l.data(), list, 4 * (size_t)n_heavy);
		d2h(off.data(), preg_off, 4 * ((size_t)n_reads + 1));
		for (int32_t p : l) { const int c = off[2 * (size_t)p + 2] - off[2 * (size_t)p]; ++heavy_census[c <= 170 ? 5 : c <= 340 ? 6 : 7]; }
	}
	// The bins of the row-parallel backward sweeps (k_seed_bwd_g): four lists of task ids by the length of the tasks' forward lists, filled by
	// the forward kernel that makes the lists (hip_fm_coop.h persistent_lanes, grant step), so that the backward launch starts with nothing in
	// front of it.  They have to exist before the forward launch, when the number of tasks is not known: each holds task_cap ids (a task is in
	// one bin at most, and ids from task_cap on are refused).  One block (hip_fm_coop.h seed_bin_list), taken from the arena by the first forward
	// launch after seed_prepare(), used by every pass and group of the batch, handed back with the seeding stage's memory.  Its first words are
	// the counters: [0..3] the bins' sizes, [4..7] k_seed_bwd_g's item counters; cleared in front of every forward launch.
	struct SeedBins { int32_t *mem = nullptr; int32_t cap = 0; };
	SeedBins seed_bins;
	bool seed_bins_on() const { return sw.seed_bwd2 == 2 && !sw.sw_simple; }
	void seed_bins_attach(SeedKArgs &A)
	{
		if (!seed_bins_on()) return;
		if (!seed_bins.mem || seed_bins.cap != A.P.task_cap) { seed_bins.mem = alloc<int32_t>(seed_bin_words(A.P.task_cap)); seed_bins.cap = A.P.task_cap; }
		memset0(seed_bins.mem, 32);
		A.bins = seed_bins.mem; A.mid = sw.seed_bwd_mid;
	}
	// opt-in record of the bins (arx_selftest_seed_bins; tests assert from it that every task is in the bin its list length names).  Everything
	// it reports is in device memory after a forward launch anyway; switched on, it is copied home after the launch: the launch's tasks
	// [t0, t0 + n) with their list lengths, the four counters, the four lists and the error word.  Switched off (everywhere else) it is one
	// untaken branch on the host per forward launch.
	struct SeedBinsRecord { int32_t t0 = 0, n = 0, cnt[4] = {0, 0, 0, 0}; uint32_t err = 0; std::vector<int32_t> task_n, bin[4]; };
	bool seed_bins_log_on = false;
	std::vector<SeedBinsRecord> seed_bins_log;
	void seed_bins_record(const SeedPools &P, int t0, int n) // n < 0: the launch made the tasks itself (first pass): as many as the task cursor says
	{
		if (!seed_bins_log_on || !seed_bins.mem) return;
		SeedBinsRecord r;
		if (n < 0) { int32_t cur[2]; d2h(cur, P.cursors, 8); n = cur[1] < P.task_cap ? cur[1] : P.task_cap; }
		r.t0 = t0; r.n = n;
		std::vector<SeedTask> tk((size_t)n);
		d2h(tk.data(), P.tasks + t0, sizeof(SeedTask) * (size_t)n);
		for (const SeedTask &k : tk) r.task_n.push_back(k.n);
		d2h(r.cnt, seed_bins.mem, 16);
		d2h(&r.err, P.err, 4);
		for (int c = 0; c < 4; ++c) {
			if (r.cnt[c] < 0 || r.cnt[c] > seed_bins.cap) throw std::runtime_error("seed_bins_record: a bin's counter is outside its list");
			r.bin[c].resize((size_t)r.cnt[c]);
			d2h(r.bin[c].data(), seed_bin_list(seed_bins.mem, c, seed_bins.cap), 4 * (size_t)r.cnt[c]);
		}
		seed_bins_log.push_back(std::move(r));
	}
	template <class K> void launch_seed_kernel(const char *nm, K kern, int n, const SeedKArgs &A, int32_t *counter, int bpc_, int chunk_ = 0, int batch_ = 0, int grant_ = 64)
	{
		if (chunk_ <= 0) chunk_ = sw.seed_chunk;
		if (batch_ <= 0) batch_ = sw.seed_batch;
		memset0(counter, 4);
		Scope sc(*this, nm, n);
		int blocks = (n + 63) / 64; if (blocks > n_cu * bpc_) blocks = n_cu * bpc_;
		start(nm, kern, dim3(blocks), dim3(64), 64 * (size_t)seed_row, A, n, counter, (batch_ & 0xff) | grant_ << 8, chunk_);
	}
	template <class F> void run_seed_fwd1(const char *nm, int n, const F &f, int32_t *counter)
	{
		if (n <= 0) return;
		if (sw.sw_simple) { launch(nm, n, f); return; }
		SeedKArgs A{f.ix, f.bases, f.base_off, f.lens, f.P, f.scratch, f.list_cap, f.first1, 0, nullptr, nullptr, 0, seed_row, seed_qn, f.read0, seed_dbg()};
		seed_bins_attach(A);
		launch_seed_kernel(nm, k_seed_fwd1, n, A, counter, seed_bpc(), 0, 0, sw.seed_grant); // (the re-seeding pass has one extension per item: no grant step of its own)
		seed_dbg_report(nm, n);
		seed_bins_record(f.P, 0, -1);
	}
	template <class F> void run_seed_fwd2(const char *nm, int n, const F &f, int32_t *counter)
	{
		if (n <= 0) return;
		if (sw.sw_simple) { launch(nm, n, f); return; }
		SeedKArgs A{f.ix, f.bases, f.base_off, f.lens, f.P, f.scratch, f.list_cap, nullptr, f.t0, nullptr, nullptr, 0, seed_row, seed_qn, 0, seed_dbg()};
		seed_bins_attach(A);
		launch_seed_kernel(nm, k_seed_fwd2, n, A, counter, seed_bpc());
		seed_dbg_report(nm, n);
		seed_bins_record(f.P, f.t0, n);
	}
	// backward sweeps: run_seed_bwd() dispatches on sw.seed_bwd2 to one function per kernel variant (switches.h has their story; all four are
	// pinned by tests/test_seed_variants_gpu.py).  A: the variant's kernel arguments; A.heavy / A.n_heavy: the list of the sweeps that are
	// finished by whole wavefronts (k_seed_bwd_wave) -- the ones longer than sw.seed_bwd_budget extensions, or too long for a row
	template <class F> void run_seed_bwd(const char *nm, int n, const F &f, int32_t *counter)
	{
		if (n <= 0) return;
		if (sw.sw_simple) { launch(nm, n, f); return; }
		int32_t *heavy = alloc<int32_t>((size_t)n + 2);
		memset0(heavy + n, 4);
		SeedKArgs A{f.ix, f.bases, f.base_off, f.lens, f.P, nullptr, 0, nullptr, f.t0, heavy, heavy + n, sw.seed_bwd_budget, seed_row, seed_qn, 0, seed_dbg()};
		if (!sw.text_bwd) A.ix.isa40 = nullptr; // ARX_TEXT_BWD=0: every sweep walked to its end (k_seed_bwd_g hands nothing to KSeedBwdTail)
		if (sw.seed_bwd2 == 3) seed_bwd_entries(nm, n, f, A, counter);
		else if (sw.seed_bwd2 == 2) seed_bwd_rows(nm, n, f, A);
		else if (sw.seed_bwd2) seed_bwd_pipelined(nm, n, f, A, counter);
		else seed_bwd_round1(nm, n, f, A, counter);
	}
	// The hand-off tail of a backward pass and its census.  wave: k_seed_bwd_wave finishes the listed sweeps; flag (may be null: the kernel
	// listed them itself) marks the tasks k_collect_heavy puts on the list first; tail: KSeedBwdTail finishes the sweeps flagged 2
	template <class F> void seed_bwd_handoff(int n, const F &f, const SeedKArgs &A, bool wave, const uint8_t *flag, bool tail, const int32_t *cnt)
	{
		if (wave) {
			Scope sc(*this, "seed_bwd_wave", n);
			if (flag) start("k_collect_heavy", k_collect_heavy, dim3((n + 255) / 256), dim3(256), 0, flag, n, f.t0, A.heavy, A.n_heavy);
			start("k_seed_bwd_wave", k_seed_bwd_wave, dim3(n_cu * 16), dim3(64), 0, A);
			if (tail) items_kernel("KSeedBwdTail", n, KSeedBwdTail{f.ix, f.bases, f.base_off, f.P.pool, f.P.tasks, f.t0, flag}, INT_MAX);
		}
		seed_census_add(n, cnt, A.n_heavy, flag);
	}
	// ARX_SEED_BWD2=3, entry-parallel sweeps (k_seed_bwd_e): one lane per list entry
	template <class F> void seed_bwd_entries(const char *nm, int n, const F &f, const SeedKArgs &A, int32_t *counter)
	{
		int32_t *ecnt = alloc<int32_t>((size_t)n + 2), *eoff = alloc<int32_t>((size_t)n + 2);
		Scope sc(*this, nm, n);
		const dim3 per_task((n + 255) / 256);
		start("k_bwd_e_count", k_bwd_e_count, per_task, dim3(256), 0, f.P.tasks, f.t0, n, ecnt);
		const int64_t total = exclusive_scan(ecnt, eoff, n); // (waits for the stream)
		BwdItem *items = alloc<BwdItem>((size_t)total + 4);
		start("k_bwd_e_expand", k_bwd_e_expand, per_task, dim3(256), 0, f.P.tasks, f.P.pool, f.t0, n, eoff, items);
		if (total > 0) {
			memset0(counter, 4);
			int64_t blocks = (total + 63) / 64; if (blocks > (int64_t)n_cu * sw.seed_bwd_e_bpc) blocks = (int64_t)n_cu * sw.seed_bwd_e_bpc;
			start("k_seed_bwd_e", k_seed_bwd_e, dim3((unsigned)blocks), dim3(64), 0, A, items, (int)total, counter, sw.seed_bwd_e_chunk);
			start("k_bwd_e_final", k_bwd_e_final, per_task, dim3(256), 0, f.P.tasks, f.P.pool, f.t0, n);
		}
		seed_dbg_report(nm, (int)total);
		seed_census_add(n, nullptr, nullptr, nullptr); // (nothing is handed on)
	}
	// ARX_SEED_BWD2=2 (the default), row-parallel sweeps (k_seed_bwd_g<FIT32>): one task per 16/32/64-lane group, lists in registers.  The tasks
	// [f.t0, f.t0 + n) are the ones the forward launch before this one gave their lists, and it has binned them (seed_bins)
	template <class F> void seed_bwd_rows(const char *nm, int n, const F &f, const SeedKArgs &A)
	{
		if (!seed_bins.mem || seed_bins.cap != f.P.task_cap) throw std::runtime_error("seed_bwd_rows: no forward launch has filled the bins");
		uint8_t *flag = alloc<uint8_t>((size_t)n + 8);
		int32_t *const cnt = seed_bins.mem;
		memset0(flag, (size_t)n);
		{
			Scope sc(*this, nm, n);
			const bool fit32 = sw.seed_fit32 && (((f.ix.L2[1] - f.ix.L2[0]) | (f.ix.L2[2] - f.ix.L2[1]) | (f.ix.L2[3] - f.ix.L2[2]) | (f.ix.L2[4] - f.ix.L2[3])) >> 32) == 0;
			const int cap = n_cu * sw.seed_bwd_bpc, b = (n + 3) / 4, blocks = b > cap ? cap : (b < 1 ? 1 : b); // four tasks per wavefront
			const size_t lds = ((4 * (size_t)seed_row + 31) & ~(size_t)31) + 64 * 32; // four reads and the lanes' exchange words
			start({"k_seed_bwd_g", nm, fit32}, fit32 ? k_seed_bwd_g<true> : k_seed_bwd_g<false>, dim3(blocks), dim3(64), lds, A, seed_bin_list(cnt, 0, seed_bins.cap), seed_bin_list(cnt, 1, seed_bins.cap), seed_bin_list(cnt, 2, seed_bins.cap), seed_bin_list(cnt, 3, seed_bins.cap), cnt, flag);
		}
		if (sw.seed_hist) { // diagnostics: forward-list lengths of this launch's tasks
			std::vector<SeedTask> ht((size_t)n);
			d2h(ht.data(), f.P.tasks + f.t0, (size_t)n * sizeof(SeedTask));
			long long hist[40] = {0};
			for (auto &k : ht) ++hist[k.n < 39 ? k.n : 39];
			fprintf(stderr, "[arx seed hist] %d tasks, list lengths 0..39+:", n);
			for (int i = 0; i < 40; ++i) fprintf(stderr, " %lld", hist[i]);
			fprintf(stderr, "\n");
		}
		if (sw.seed_stats) { int32_t h[4]; d2h(h, cnt, 16); fprintf(stderr, "[arx seed stats] backward tasks by list length: <= 16: %d, <= %d: %d, <= 32: %d, longer: %d\n", h[0], sw.seed_bwd_mid, h[1], h[2], h[3]); }
		seed_dbg_report(nm, n);
		// the tail: the sweeps k_seed_bwd_g left at a row of one interval with one occurrence (text mode)
		seed_bwd_handoff(n, f, A, /* wave */ true, flag, /* tail */ A.ix.isa40 != nullptr, cnt);
	}
	// ARX_SEED_BWD2=1, pipelined refills (k_seed_bwd2): one lane per task, one wait on memory per iteration
	template <class F> void seed_bwd_pipelined(const char *nm, int n, const F &f, const SeedKArgs &A, int32_t *counter)
	{
		uint8_t *flag = alloc<uint8_t>((size_t)n + 8);
		memset0(flag, (size_t)n);
		memset0(counter, 4);
		{
			Scope sc(*this, nm, n);
			int blocks = (n + 63) / 64; if (blocks > n_cu * seed_bpc()) blocks = n_cu * seed_bpc();
			start("k_seed_bwd2", k_seed_bwd2, dim3(blocks), dim3(64), 64 * (size_t)seed_row, A, n, counter, sw.seed_bwd_chunk, flag);
		}
		seed_dbg_report(nm, n);
		seed_bwd_handoff(n, f, A, /* wave */ sw.seed_bwd_budget > 0, flag, /* tail */ false, /* no bins */ nullptr);
	}
	// ARX_SEED_BWD2=0, round 1's kernel (k_seed_bwd): one lane per task, it lists the sweeps past their budget itself
	template <class F> void seed_bwd_round1(const char *nm, int n, const F &f, const SeedKArgs &A, int32_t *counter)
	{
		launch_seed_kernel(nm, k_seed_bwd, n, A, counter, seed_bpc(), sw.seed_bwd_chunk, sw.seed_bwd_batch);
		seed_dbg_report(nm, n);
		seed_bwd_handoff(n, f, A, /* wave */ sw.seed_bwd_budget > 0, /* listed by the kernel */ nullptr, /* tail */ false, /* no bins */ nullptr);
	}
	template <class F> void run_seed_strat(const char *nm, int n, const F &f, int32_t *counter)
	{
		if (n <= 0) return;
		if (sw.sw_simple) { launch(nm, n, f); return; }
		memset0(counter, 4);
		Scope sc(*this, nm, n);
		StratArgs A{f.ix, f.bases, f.base_off, f.lens, f.strat, f.n_strat, seed_row, seed_qn};
		int blocks = (n + 63) / 64; if (blocks > n_cu * strat_bpc()) blocks = n_cu * strat_bpc();
		start("k_strat_dyn", k_strat_dyn, dim3(blocks), dim3(64), 64 * (size_t)seed_row, A, n, counter, sw.seed_chunk);
	}
	// locate: persistent lanes with wave-level work distribution (hip_fm_coop.h); 32 waves per CU to cover the miss latency
	template <class F> void run_locate(const char *nm, int n, const F &f, int32_t *counter)
	{
		if (n <= 0) return;
		if (sw.sw_simple) { launch(nm, n, f); return; }
		if (f.ix.sa40) { launch_wide(nm, n, f); return; } // the whole suffix array is resident: one load per occurrence, no walk to balance
		memset0(counter, 4);
		Scope sc(*this, nm, n);
		int blocks = (n + 255) / 256; if (blocks > n_cu * 8) blocks = n_cu * 8;
		start("k_locate_dyn", k_locate_dyn, dim3(blocks), dim3(256), 0, f.ix, f.occ_seed, n, counter);
	}
	// banded extension: 16 lanes per extension (hip_sw_coop.h); the query-length classes share one launch
	using ExtKernel = void (*)(IndexView, const uint8_t *, const ExtTask *, ExtRes *, int);
	template <class F> void run_extend(const char *nm, const int32_t *n_class, int stride, const F &f)
	{
		int total = 0;
		for (int c = 0; c < EXT_CLASSES; ++c) total += n_class[c];
		if (total <= 0) return;
		if (sw.sw_simple) {
			for (int c = 0; c < EXT_CLASSES; ++c) { F fc = f; fc.tasks = f.tasks + (size_t)c * stride; launch_rows(nm, n_class[c], fc, MAX_READ_LEN + 2); }
			return;
		}
		if (total >= sw.ext_merge_below) { // big round: one launch per class, each at the occupancy its own register tiling allows
			for (int c = 0; c < EXT_CLASSES; ++c) {
				const int nc = n_class[c];
				if (nc <= 0) continue;
				Scope sc(*this, nm, nc);
				const ExtTask *tk = f.tasks + (size_t)c * stride;
				// per class: round 2's kernel on the same class lists (sw.ext_old), and this round's at the class's own register tiling
				static constexpr ExtKernel by_class[EXT_CLASSES][2] = {{k_extend_b16<4, true>, k_extend_b16<2, false>}, {k_extend_b16<4, true>, k_extend_b16<3, false>},
					{k_extend_b16<4, true>, k_extend_b16<4, false>}, {k_extend_b16<7, true>, k_extend_b16<6, false>}, {k_extend_b16<10, true>, k_extend_b16<8, false>},
					{k_extend_b16<10, true>, k_extend_b16<10, false>}, {k_extend_b16<16, true>, k_extend_b16<16, false>}};
				start({sw.ext_old ? "k_extend_b16<old>" : "k_extend_b16", nm, c}, by_class[c][sw.ext_old ? 0 : 1], dim3(coop_blocks(nc)), dim3(64), 0, f.ix, f.bases, tk, f.res, nc);
			}
			return;
		}
		Scope sc(*this, nm, total);
		ExtClassShape sh;
		const int cap = n_cu * sw.coop_bpc;
		int blocks = 0;
		for (int c = 0; c < EXT_CLASSES; ++c) {
			sh.n[c] = n_class[c];
			int nb = (n_class[c] + 3) / 4;
			if (nb > 0 && (total + 3) / 4 > cap) { nb = (int)((int64_t)nb * cap / ((total + 3) / 4)); if (nb < 1) nb = 1; } // share the grid cap by class size
			sh.nb[c] = nb; blocks += nb;
		}
		start({"k_extend_classes_b", nm, sw.ext_old}, sw.ext_old ? k_extend_classes_b<true> : k_extend_classes_b<false>, dim3(blocks), dim3(64), 0, f.ix, f.bases, f.tasks, stride, f.res, sh);
	}
	// CIGARs of the gapped regions: 16 lanes per region (hip_nw_coop.h); f is pipeline.h's KReg2Aln
	using NwKernel = void (*)(NwArgs, int, const int32_t *);
	const int32_t *nw_n_punt = nullptr; // the last run_reg2aln_nw's punt counter on the device (null: it kept none)
	int nw_punts() { if (!nw_n_punt) return -1; int32_t v = 0; d2h(&v, nw_n_punt, 4); return v; } // Pipeline::reg2aln_census
	template <class F> void run_reg2aln_nw(const char *nm, int n, const int32_t *n_class, const F &f, uint8_t *zbuf, const int32_t *z_off)
	{
		nw_n_punt = nullptr;
		if (n <= 0) return;
		if (sw.sw_simple) { launch_small(nm, n, f); return; }
		// one launch per band class: the four groups of a wavefront then run the same tiling, and the class kernel holds only the tilings the
		// class can need (its own and the doubled band's): 5 / 4 / 3 / 2 / 2 wavefronts per SIMD instead of 2 for all
		int32_t *punt = alloc<int32_t>((size_t)n + 4), *n_punt = punt + n;
		memset0(n_punt, 16);
		nw_n_punt = n_punt;
		auto run_class = [&](int c) {
			const int nc = n_class[c];
			if (nc <= 0) return;
			Scope sc(*this, nm, nc);
			NwArgs A{f.ix, f.bases, f.base_off, f.lens, f.preg_off, f.n_regs, f.n_reads, f.pregs, f.alns, f.cig, f.cig_w, zbuf, z_off, f.nw_list, f.err,
			         f.class_list + (size_t)c * f.class_stride, punt, n_punt};
			static constexpr NwKernel by_class[NW_CLASSES] = {k_reg2aln_nw_g16<1, 2>, k_reg2aln_nw_g16<2, 4>, k_reg2aln_nw_g16<4, 8>, k_reg2aln_nw_g16<8, 16>, k_reg2aln_nw_g16<16, 16>};
			start({"k_reg2aln_nw_g16", nm, c}, by_class[c], dim3(coop_blocks(nc)), dim3(64), 0, A, nc, nullptr);
		};
		// class 2 (<4, 8>) beside the others: 3.4 ms against 0.9 + 2.5 + 1.4 ms per batch for classes 0, 1 and 3 (class 4 is all but empty), the
		// most even split of the measured class times.  A class touches its own regions' slots and appends to the punt list by atomics; the
		// join comes before the launch that reads n_punt
		constexpr int side_class = 2;
		if (aux_on(AUX_NW)) {
			if (n_class[side_class] > 0) on_aux(AUX_NW, [&]() { run_class(side_class); });
			for (int c = 0; c < NW_CLASSES; ++c) if (c != side_class) run_class(c);
		} else for (int c = 0; c < NW_CLASSES; ++c) run_class(c); // one stream: the classes in their order
		aux_join();
		{ // what the class kernels handed on (a third band, or a doubled band past the class's second tiling): all tilings, length read on the device
			Scope sc(*this, nm, 0);
			NwArgs A{f.ix, f.bases, f.base_off, f.lens, f.preg_off, f.n_regs, f.n_reads, f.pregs, f.alns, f.cig, f.cig_w, zbuf, z_off, f.nw_list, f.err, punt, punt, n_punt + 1};
			start({"k_reg2aln_nw_g16<1, 16>", "punted"}, k_reg2aln_nw_g16<1, 16>, dim3(n_cu * 2), dim3(64), 0, A, 0, n_punt);
		}
	}
	template <class F> void launch_rows(const char *nm, int n, const F &f, int words_per_thread)
	{
		if (n <= 0) return;
		Scope sc(*this, nm, n);
		int blocks = (n + 63) / 64; if (blocks > max_blocks()) blocks = max_blocks();
		size_t lds = (size_t)words_per_thread * 64 * 4;
		start({"k_rows", nm}, k_rows<F>, dim3(blocks), dim3(64), lds, f, n);
	}
	// out[0..n] = exclusive prefix sums of in[0..n); returns the total as int64
	int64_t exclusive_scan(const int32_t *in, int32_t *out, int n)
	{
		Scope sc(*this, "scan", n);
		size_t need = 0;
		hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, n, stream);
		size_t need2 = 0;
		hipcub::TransformInputIterator<int64_t, CastI64, const int32_t *> it(in, CastI64());
		hipcub::DeviceReduce::Sum(nullptr, need2, it, d_total.as<int64_t>(), n, stream);
		void *tmp = scan_tmp.get(need2 > need ? need2 : need); // one scratch for both
		size_t nb = scan_tmp.buf.bytes;
		ARX_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, nb, in, out, n, stream));
		nb = scan_tmp.buf.bytes;
		ARX_HIP_CHECK(hipcub::DeviceReduce::Sum(tmp, nb, it, d_total.as<int64_t>(), n, stream));
		int64_t total = 0;
		d2h(&total, d_total.p, 8);
		int32_t t32 = (int32_t)(total < ((int64_t)1 << 31) ? total : 0x7fffffff);
		ARX_HIP_CHECK(hipMemcpyAsync(out + n, &t32, 4, hipMemcpyHostToDevice, stream));
		ARX_HIP_CHECK(hipStreamSynchronize(stream));
		return total;
	}
};

} // namespace arx

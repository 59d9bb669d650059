// hip_gunzip.h -- dev_gunzip.h on the GPU: the chunked inflate of one plain DEFLATE stream behind arx_selftest_gunzip.  Included by
// arx_bgzf.hip, next to hip_inflate.h.  GzHip is the backend gunzip_host.h's reader drives: per slab of compressed bytes one decode(), which ends
// with the sizes, and one resolve() to the place the caller has made for the text.  Each of the two also exists as an enqueue half and a wait
// half (decode_begin / decode_end, resolve_begin / resolve_end) for the device feeder, which keeps two files' launches in flight at once.
//
//   k_gunzip_find     one wavefront per chunk: its candidate (dev_gunzip.h: gz_chunk_find).  About 13 KB of LDS
//   k_gunzip_decode   one wavefront per chunk with a candidate: its blocks as 16-bit symbols into its span of the staging buffer; the ring of
//                     GZ_RING symbols and the decode tables in LDS (about 80 KB, two wavefronts a CU: the LDS opt-in of k_bgzf_inflate)
//   k_gunzip_windows  one workgroup: the accepted chain (one lane), then the window behind every accepted chunk, in order
//   k_gunzip_resolve  one workgroup per accepted chunk: its bytes at their final place, the markers replaced through the window in front of it,
//                     and their CRC-32
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "hip_launch.h"
#include "hip_res.h"
#include "hip_inflate.h" // InfHipDrv
#include "dev_gunzip.h"
#include "gunzip_host.h"

namespace arx {

constexpr int GZ_WINDOW_THREADS = 1024, GZ_RESOLVE_THREADS = 256;

static __global__ void __launch_bounds__(INF_LANES) k_gunzip_find(const uint8_t *src, int clen, int chunk_bytes, int start_bit, int n_chunks, GzChunk *chunks)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t lds_gunzip_find[];
	const int k = blockIdx.x;
	if (k >= n_chunks) return;
	GzWork w;
	gz_carve(w, lds_gunzip_find); // (the ring lies behind what this kernel is given, and is not touched)
	InfHipDrv drv{(int)threadIdx.x};
	GzChunk c;
	gz_chunk_find(drv, w, src, clen, chunk_bytes, start_bit, k, c);
	if (threadIdx.x == 0) chunks[k] = c;
}

static __global__ void __launch_bounds__(INF_LANES) k_gunzip_decode(const uint8_t *src, int clen, int expand, int n_chunks, GzChunk *chunks, uint16_t *stage)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t lds_gunzip[];
	const int k = blockIdx.x;
	if (k >= n_chunks) return;
	GzWork w;
	gz_carve(w, lds_gunzip);
	InfHipDrv drv{(int)threadIdx.x};
	gz_chunk_decode(drv, w, src, clen, expand, k, n_chunks, chunks, stage);
}

// windows: (n_chunks + 1) x GZ_WIN bytes, the first the carried window
static __global__ void __launch_bounds__(GZ_WINDOW_THREADS) k_gunzip_windows(GzChunk *chunks, int n_chunks, int have, const uint16_t *stage, uint8_t *windows, GzChain *chain)
{
	if (threadIdx.x == 0) gz_chain(chunks, n_chunks, have, *chain);
	__syncthreads(); // (workgroup scope: what lane 0 wrote to global memory is read by the other lanes of this workgroup only)
	const int n = chain->n_accepted;
	for (int m = 0, k = 0; m < n && k < n_chunks; ++m) {
		const GzChunk &c = chunks[k];
		const uint16_t *sym = stage + c.stage_off;
		const uint8_t *prev = windows + (size_t)m * GZ_WIN;
		uint8_t *next = windows + (size_t)(m + 1) * GZ_WIN;
		if (c.have < GZ_WIN) { // the first 32 KiB of a member: does a marker reach in front of it?
			int bad = 0;
			for (int64_t i = threadIdx.x; i < c.count; i += GZ_WINDOW_THREADS) bad += gz_bad_marker_at(sym, c.have, i);
			if (bad) atomicAdd(&chunks[k].bad_markers, bad); // (0 since the search for candidates)
		}
		for (int i = threadIdx.x; i < GZ_WIN; i += GZ_WINDOW_THREADS) gz_window_at(prev, next, sym, c.count, i);
		k = c.next;
		__syncthreads(); // the next window reads this one
	}
}

static __global__ void __launch_bounds__(GZ_RESOLVE_THREADS) k_gunzip_resolve(GzChunk *chunks, int n_chunks, const uint16_t *stage, const uint8_t *windows, uint8_t *text)
{
	__shared__ uint32_t crc_tab[256], x2n[32], part[GZ_RESOLVE_THREADS];
	__shared__ int n_marker;
	const int k = blockIdx.x, t = threadIdx.x;
	if (k >= n_chunks) return;
	const GzChunk c = chunks[k];
	if (!(c.flags & GZ_F_ACCEPTED)) return;
	if (t == 0) n_marker = 0;
	gz_crc_tables(crc_tab, x2n, t, GZ_RESOLVE_THREADS);
	__syncthreads();
	const uint8_t *win = windows + (size_t)c.order * GZ_WIN;
	const uint16_t *sym = stage + c.stage_off;
	uint8_t *out = text + c.text_off;
	int markers = 0;
	for (int64_t i = t; i < c.count; i += GZ_RESOLVE_THREADS) markers += gz_resolve_at(win, sym, out, i);
	if (markers) atomicAdd(&n_marker, markers);
	__syncthreads(); // the bytes this workgroup wrote are read back by it
	part[t] = gz_crc_part(crc_tab, x2n, out, c.count, t, GZ_RESOLVE_THREADS);
	__syncthreads();
	if (t == 0) {
		uint32_t crc = 0;
		for (int i = 0; i < GZ_RESOLVE_THREADS; ++i) crc ^= part[i];
		chunks[k].crc = crc; chunks[k].markers = n_marker;
	}
}

// gunzip_host.h's backend on a device: every buffer is kept from launch to launch and grown on demand.  st: the caller's stream, on which the
// place the text goes to is valid
struct GzHip {
	hipStream_t st = nullptr;
	DevBuf d_src, d_chunks, d_stage, d_windows, d_chain;
	Event ev[5];
	int n = 0;
	void init(hipStream_t stream)
	{
		st = stream;
		for (Event &e : ev) e.create(hipEventDefault);
		d_chain.alloc(sizeof(GzChain));
	}
	static void room(DevBuf &b, size_t bytes) { if (!b.p || b.bytes < bytes) b.alloc(bytes + (bytes >> 2)); }
	// find, decode, windows: the chunks and the chain, and with them the size of the text.  In two halves, so that a caller with several files
	// (device_feeder.h) has every file's launches in flight before it waits for any: decode_begin enqueues the upload and the three kernels and
	// returns; decode_end brings the chunks and the chain home and waits.  (The copies home are the wait half's: into pageable memory the
	// runtime makes them wait for the stream.)  decode() is the two in a row
	int64_t stage_n = 0;
	void decode_begin(const uint8_t *src, int clen, int start_bit, const uint8_t *window, int have, int chunk_bytes, int expand)
	{
		n = (int)(((int64_t)clen + chunk_bytes - 1) / chunk_bytes);
		stage_n = gz_stage_at(8 * (int64_t)clen, expand);
		room(d_src, (size_t)clen); room(d_chunks, sizeof(GzChunk) * (size_t)n); room(d_stage, 2 * (size_t)stage_n); room(d_windows, (size_t)(n + 1) * GZ_WIN);
		GzChunk *chunks = d_chunks.as<GzChunk>();
		ARX_HIP_CHECK(hipMemcpyAsync(d_src.p, src, (size_t)clen, hipMemcpyHostToDevice, st));
		ARX_HIP_CHECK(hipMemcpyAsync(d_windows.p, window, GZ_WIN, hipMemcpyHostToDevice, st));
		// per device and cheap; set on every launch rather than remembered per device
		ARX_HIP_CHECK(hipFuncSetAttribute((const void *)k_gunzip_decode, hipFuncAttributeMaxDynamicSharedMemorySize, GZ_WORK_BYTES));
		ARX_HIP_CHECK(hipEventRecord(ev[0], st));
		hip_launch("k_gunzip_find", k_gunzip_find, dim3(n), dim3(INF_LANES), GZ_FIND_BYTES, st, d_src.as<uint8_t>(), clen, chunk_bytes, start_bit, n, chunks);
		ARX_HIP_CHECK(hipEventRecord(ev[1], st));
		hip_launch("k_gunzip_decode", k_gunzip_decode, dim3(n), dim3(INF_LANES), GZ_WORK_BYTES, st, d_src.as<uint8_t>(), clen, expand, n, chunks, d_stage.as<uint16_t>());
		ARX_HIP_CHECK(hipEventRecord(ev[2], st));
		hip_launch("k_gunzip_windows", k_gunzip_windows, dim3(1), dim3(GZ_WINDOW_THREADS), 0, st, chunks, n, have, d_stage.as<uint16_t>(), d_windows.as<uint8_t>(), d_chain.as<GzChain>());
		ARX_HIP_CHECK(hipEventRecord(ev[3], st));
	}
	void decode_end(GzLaunch &L)
	{
		L.chunks.resize((size_t)n);
		ARX_HIP_CHECK(hipMemcpyAsync(L.chunks.data(), d_chunks.p, sizeof(GzChunk) * (size_t)n, hipMemcpyDeviceToHost, st));
		ARX_HIP_CHECK(hipMemcpyAsync(&L.chain, d_chain.p, sizeof(GzChain), hipMemcpyDeviceToHost, st));
		ARX_HIP_CHECK(hipStreamSynchronize(st));
		if (L.chain.n_accepted < 0 || L.chain.n_accepted > n || L.chain.text_bytes < 0 || L.chain.text_bytes > stage_n) throw HipError("k_gunzip_windows: a chain outside the launch");
		for (int p = 0; p < 3; ++p) {
			float ms = 0;
			ARX_HIP_CHECK(hipEventElapsedTime(&ms, ev[p], ev[p + 1]));
			L.us[p] = 1000.0 * ms;
		}
		L.us[3] = 0;
	}
	void decode(const uint8_t *src, int clen, int start_bit, const uint8_t *window, int have, int chunk_bytes, int expand, GzLaunch &L)
	{
		decode_begin(src, clen, start_bit, window, have, chunk_bytes, expand);
		decode_end(L);
	}
	// resolve: the accepted chunks' bytes to text[0, L.chain.text_bytes) in device memory, their CRCs, and the window behind them; in the same
	// two halves.  Where the place of the text was made on another stream (`after`), the kernel waits for what that stream holds (evo[0]), and
	// that stream for the kernel (evo[1]): what it is given next reads the text
	Event evo[2];
	void resolve_begin(GzLaunch &, uint8_t *text, hipStream_t after = nullptr)
	{
		if (after) {
			if (!evo[0].e) for (Event &e : evo) e.create(hipEventDisableTiming);
			ARX_HIP_CHECK(hipEventRecord(evo[0], after));
			ARX_HIP_CHECK(hipStreamWaitEvent(st, evo[0], 0));
		}
		ARX_HIP_CHECK(hipEventRecord(ev[3], st));
		hip_launch("k_gunzip_resolve", k_gunzip_resolve, dim3(n), dim3(GZ_RESOLVE_THREADS), 0, st, d_chunks.as<GzChunk>(), n, d_stage.as<uint16_t>(), d_windows.as<uint8_t>(), text);
		ARX_HIP_CHECK(hipEventRecord(ev[4], st));
		if (after) {
			ARX_HIP_CHECK(hipEventRecord(evo[1], st));
			ARX_HIP_CHECK(hipStreamWaitEvent(after, evo[1], 0));
		}
	}
	void resolve_end(GzLaunch &L)
	{
		ARX_HIP_CHECK(hipMemcpyAsync(L.chunks.data(), d_chunks.p, sizeof(GzChunk) * (size_t)n, hipMemcpyDeviceToHost, st));
		ARX_HIP_CHECK(hipMemcpyAsync(L.window, d_windows.as<uint8_t>() + (size_t)L.chain.n_accepted * GZ_WIN, GZ_WIN, hipMemcpyDeviceToHost, st));
		ARX_HIP_CHECK(hipStreamSynchronize(st));
		float ms = 0;
		ARX_HIP_CHECK(hipEventElapsedTime(&ms, ev[3], ev[4]));
		L.us[3] = 1000.0 * ms;
	}
	void resolve(GzLaunch &L, uint8_t *text)
	{
		resolve_begin(L, text);
		resolve_end(L);
	}
	void upload(uint8_t *dst, const uint8_t *host, size_t bytes)
	{
		if (!bytes) return;
		ARX_HIP_CHECK(hipMemcpyAsync(dst, host, bytes, hipMemcpyHostToDevice, st));
		ARX_HIP_CHECK(hipStreamSynchronize(st)); // the host's piece is written anew
	}
};

} // namespace arx

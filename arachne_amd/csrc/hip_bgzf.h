// hip_bgzf.h -- dev_bgzf.h on the GPU, and the device compressor behind BamSink's seam (bam_sink.h: BlockCompressor).
//
//   k_bgzf_deflate   one workgroup of BGZF_LANES lanes per BGZF block: input and tables in LDS (about 92 KB), the token array in a scratch row
//                    of the workgroup's own; writes the raw DEFLATE stream into the block's 64 KiB slice and four words of meta
//   k_bgzf_frame     one workgroup per block: the 18-byte BGZF header, the stream, CRC-32 and ISIZE, packed back to back in file order (the
//                    bytes BamSink::deflate_block frames a block with); a block's offset is the sum of the framed sizes in front of it
//
// DeviceBgzf owns (through the types of hip_res.h) two streams, two page-locked staging pairs and the device buffers of two groups of at most GROUP blocks, allocated once
// (about 64 MB of page-locked and 100 MB of device memory: one per device for the life of the process, see arx_bgzf.hip).
// run() takes the blocks of one flush in groups: while group g is uploaded, compressed, framed and its sizes come back, the framed bytes of
// group g - 1 are downloaded and written.  Blocks reach the sink in order.  run_device() is run() for a stream that is in device memory already
// (arx_bam_write_encoded_device: the records phase's output, dev_records.h): only where a group's input comes from differs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>
#include "hip_res.h"
#include "dev_bgzf.h"
#include "hip_block.h"
#include "bam_sink.h"

namespace arx {

struct BgzfHipDrv { // dev_bgzf.h's driver on a workgroup
	HipBlockT<BGZF_LANES, 1> blk;
	template <class F> __device__ __forceinline__ void lanes(F f) { f(blk.tid); __syncthreads(); }
	__device__ __forceinline__ void scan(const int32_t *in, int32_t *out, int n) { blk.exclusive_scan(in, out, n); }
};

constexpr int BGZF_TOK_ROW = BGZF_IN + 8; // uint16 entries of a workgroup's token row

static __global__ void __launch_bounds__(BGZF_LANES) k_bgzf_deflate(const uint8_t *src, int64_t total, int n_blocks, uint16_t *tok, uint32_t *out, uint32_t *meta)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t lds_bgzf[];
	__shared__ int32_t l32[BGZF_LANES + 1];
	BgzfWork w;
	bgzf_carve(w, lds_bgzf, tok + (size_t)blockIdx.x * BGZF_TOK_ROW);
	BgzfHipDrv drv{{(int)threadIdx.x, nullptr, l32, nullptr, nullptr}}; // only exclusive_scan is used: it needs l32 alone (no l64, no sort buffers)
	drv.lanes([&](int lane) { bgzf_tables(w, lane); });
	drv.lanes([&](int lane) { bgzf_shift_table(w, lane); });
	// uniform over the workgroup.  With a grid of min(CUs, GROUP) workgroups and at most GROUP blocks per launch a workgroup takes a second
	// block only on a device with fewer than GROUP CUs (the host simulator runs every block through one BgzfWork)
	for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
		const int64_t b0 = (int64_t)b * BGZF_IN;
		const int n = total - b0 < BGZF_IN ? (int)(total - b0) : BGZF_IN;
		bgzf_block(drv, w, src + b0, n, out + (size_t)b * (BGZF_OUT_SLICE / 4), meta + 4 * (size_t)b);
	}
}

static __global__ void __launch_bounds__(256) k_bgzf_frame(const uint32_t *slices, const uint32_t *meta, int n_blocks, uint8_t *packed)
{
	__shared__ unsigned int lds_off;
	const int b = blockIdx.x, tid = threadIdx.x;
	if (tid == 0) lds_off = 0;
	__syncthreads();
	unsigned int part = 0;
	for (int k = tid; k < b; k += 256) part += meta[4 * k] + 26;
	if (part) atomicAdd(&lds_off, part);
	__syncthreads();
	const uint32_t clen = meta[4 * b], crc = meta[4 * b + 1], isize = meta[4 * b + 3], bsize = 18 + clen + 8 - 1;
	uint8_t *o = packed + lds_off; // at most n_blocks * 65536 bytes: clen <= 5 + 65280
	const uint8_t *s = (const uint8_t *)(slices + (size_t)b * (BGZF_OUT_SLICE / 4));
	if (tid < 18) {
		const uint8_t hdr[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8)};
		o[tid] = hdr[tid];
	} else if (tid < 26) {
		const int k = tid - 18;
		o[18 + clen + k] = (uint8_t)((k < 4 ? crc : isize) >> (8 * (k & 3)));
	}
	for (uint32_t i = tid; i < clen; i += 256) o[18 + i] = s[i];
}

struct DeviceBgzf : BlockCompressor {
	static constexpr int GROUP = 256; // blocks of a group: 16 MiB each way
	int dev = -1, n_cu = 256, grid = 0;
	bool ready = false;
	// what it holds (hip_res.h).  The streams first: members die in reverse order, so a stream has ended (its destructor waits) after nothing but
	// its own events and buffers were freed, and those are only freed once the flush that used them has returned
	Stream st[2];
	Event ev_meta[2], ev_pay[2];
	PinnedBuf h_in[2], h_out[2], h_meta[2];
	DevBuf d_in[2], d_slices[2], d_packed[2], d_meta[2], d_tok[2];
	int64_t n_form[3] = {0, 0, 0}; // blocks that went out stored, fixed, dynamic
	std::mutex mu;                 // the writers of one device share one compressor (arx_bgzf.hip): a flush at a time

	void init(int device)
	{
		select_device(device, "no HIP device visible: the device BAM sink needs an MI355X (there is no CPU fallback)", "device index out of range");
		dev = device;
		hipDeviceProp_t p;
		ARX_HIP_CHECK(hipGetDeviceProperties(&p, dev));
		n_cu = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
		grid = n_cu < GROUP ? n_cu : GROUP; // one workgroup per CU: its LDS does not leave room for two
		ARX_HIP_CHECK(hipFuncSetAttribute((const void *)k_bgzf_deflate, hipFuncAttributeMaxDynamicSharedMemorySize, BGZF_WORK_BYTES));
		for (int s = 0; s < 2; ++s) {
			st[s].create();
			ev_meta[s].create(hipEventDisableTiming); ev_pay[s].create(hipEventDisableTiming);
			h_in[s].alloc((size_t)GROUP * BGZF_IN); h_out[s].alloc((size_t)GROUP * BGZF_OUT_SLICE); h_meta[s].alloc((size_t)GROUP * 16);
			d_in[s].alloc((size_t)GROUP * BGZF_IN); d_slices[s].alloc((size_t)GROUP * BGZF_OUT_SLICE); d_packed[s].alloc((size_t)GROUP * BGZF_OUT_SLICE);
			d_meta[s].alloc((size_t)GROUP * 16); d_tok[s].alloc((size_t)grid * BGZF_TOK_ROW * 2);
		}
		ready = true;
	}
	~DeviceBgzf() override { if (dev >= 0) (void)hipSetDevice(dev); } // (the members are this device's)

	// group g of the flush: its input into d_in[s] (stage(s, b0, bytes) enqueues that on st[s]), the two kernels, the sizes on their way back
	template <class Stage> void submit(size_t total, size_t g, Stage stage)
	{
		const int s = (int)(g & 1);
		const size_t b0 = g * GROUP * (size_t)BGZF_IN, bytes = total - b0 < (size_t)GROUP * BGZF_IN ? total - b0 : (size_t)GROUP * BGZF_IN;
		const int nb = (int)((bytes + BGZF_IN - 1) / BGZF_IN);
		stage(s, b0, bytes);
		hip_launch("k_bgzf_deflate", k_bgzf_deflate, dim3(nb < grid ? nb : grid), dim3(BGZF_LANES), BGZF_WORK_BYTES, st[s], d_in[s].as<uint8_t>(), bytes, nb, d_tok[s].as<uint16_t>(), d_slices[s].as<uint32_t>(), d_meta[s].as<uint32_t>());
		hip_launch("k_bgzf_frame", k_bgzf_frame, dim3(nb), dim3(256), 0, st[s], d_slices[s].as<uint32_t>(), d_meta[s].as<uint32_t>(), nb, d_packed[s].as<uint8_t>());
		ARX_HIP_CHECK(hipMemcpyAsync(h_meta[s].p, d_meta[s].p, (size_t)nb * 16, hipMemcpyDeviceToHost, st[s]));
		ARX_HIP_CHECK(hipEventRecord(ev_meta[s], st[s]));
	}
	// the sizes of group g are known: its framed bytes on their way back -> their number.  sizes: null, or where every block's framed size is appended
	size_t fetch(size_t g, int nb, std::vector<int64_t> *sizes)
	{
		const int s = (int)(g & 1);
		ARX_HIP_CHECK(hipEventSynchronize(ev_meta[s]));
		size_t bytes = 0;
		for (int b = 0; b < nb; ++b) {
			const uint32_t *m = h_meta[s].as<uint32_t>() + 4 * (size_t)b;
			if (m[0] > 5u + BGZF_IN || m[2] > 2u) throw std::runtime_error("the BGZF kernel reported an impossible block");
			bytes += m[0] + 26; ++n_form[m[2]];
			if (sizes) sizes->push_back((int64_t)m[0] + 26);
		}
		ARX_HIP_CHECK(hipMemcpyAsync(h_out[s].p, d_packed[s].p, bytes, hipMemcpyDeviceToHost, st[s]));
		ARX_HIP_CHECK(hipEventRecord(ev_pay[s], st[s]));
		return bytes;
	}

	// sink(bytes, n): n framed bytes, in order; stage: where a group's input comes from (submit)
	template <class Stage, class Sink> void compress_from(size_t total, Stage stage, Sink sink, std::vector<int64_t> *sizes = nullptr)
	{
		if (!ready) throw std::runtime_error("the device compressor is not initialised");
		if (!total) return;
		ARX_HIP_CHECK(hipSetDevice(dev)); // the current device is per host thread and is left set: every entry of the library that touches the GPU binds its own first
		const size_t per = (size_t)GROUP * BGZF_IN, ng = (total + per - 1) / per;
		auto blocks_of = [&](size_t g) { const size_t bytes = total - g * per < per ? total - g * per : per; return (int)((bytes + BGZF_IN - 1) / BGZF_IN); };
		auto drain = [&](size_t g) {
			const size_t bytes = fetch(g, blocks_of(g), sizes);
			ARX_HIP_CHECK(hipEventSynchronize(ev_pay[g & 1]));
			sink(h_out[g & 1].as<uint8_t>(), bytes);
		};
		try {
			submit(total, 0, stage);
			for (size_t g = 1; g < ng; ++g) { submit(total, g, stage); drain(g - 1); }
			drain(ng - 1);
		} catch (...) {
			(void)hipStreamSynchronize(st[0]); (void)hipStreamSynchronize(st[1]); // nothing of this flush stays in flight
			throw;
		}
	}
	// from host memory: through the page-locked staging of the group's stream
	template <class Sink> void compress(const uint8_t *src, size_t total, Sink sink, std::vector<int64_t> *sizes = nullptr)
	{
		compress_from(total, [&](int s, size_t b0, size_t bytes) {
			memcpy(h_in[s].p, src + b0, bytes);
			ARX_HIP_CHECK(hipMemcpyAsync(d_in[s].p, h_in[s].p, bytes, hipMemcpyHostToDevice, st[s]));
		}, sink, sizes);
	}

	bool run(const uint8_t *src, size_t total, FILE *f, int64_t &bytes_out, std::string &error, std::vector<int64_t> *sizes) override
	{
		try {
			std::lock_guard<std::mutex> lock(mu);
			bool ok = true;
			compress(src, total, [&](const uint8_t *p, size_t n) {
				if (ok && fwrite(p, 1, n, f) != n) { ok = false; error = "write failed"; }
				if (ok) bytes_out += (int64_t)n;
			}, sizes);
			return ok;
		} catch (const std::exception &e) {
			error = e.what();
			return false;
		}
	}
	// arx_bam_write_encoded_device: what is compressed is carry[0, n_carry) (host memory: the sink's pending bytes, fewer than a block) followed
	// by d_stream[0, n_bytes) (device memory of this device, complete).  Every whole block of that concatenation goes through the same groups,
	// kernels and framing as run(): the carry goes up to the front of group 0's input, the group's share of d_stream follows device to device.
	// The tail short of a block is left in `tail` (the sink's next carry).  Returns when the blocks are written.  sizes: as run()'s
	bool run_device(const uint8_t *carry, size_t n_carry, const uint8_t *d_stream, size_t n_bytes, FILE *f, int64_t &bytes_out, size_t &n_blocks, std::vector<uint8_t> &tail,
	                std::string &error, std::vector<int64_t> *sizes = nullptr)
	{
		try {
			if (n_carry >= (size_t)BGZF_IN) throw std::runtime_error("the device sink's carry is a whole block");
			std::lock_guard<std::mutex> lock(mu);
			const size_t total = n_carry + n_bytes, nb = total / BGZF_IN, used = nb * (size_t)BGZF_IN;
			bool ok = true;
			compress_from(used, [&](int s, size_t b0, size_t bytes) {
				size_t c = 0; // bytes of the group that come from the carry (group 0 only: the carry is shorter than a block)
				if (b0 < n_carry) {
					c = n_carry - b0 < bytes ? n_carry - b0 : bytes;
					memcpy(h_in[s].p, carry + b0, c);
					ARX_HIP_CHECK(hipMemcpyAsync(d_in[s].p, h_in[s].p, c, hipMemcpyHostToDevice, st[s]));
				}
				if (bytes > c) ARX_HIP_CHECK(hipMemcpyAsync(d_in[s].as<uint8_t>() + c, d_stream + (b0 + c - n_carry), bytes - c, hipMemcpyDeviceToDevice, st[s]));
			}, [&](const uint8_t *p, size_t n) {
				if (ok && fwrite(p, 1, n, f) != n) { ok = false; error = "write failed"; }
				if (ok) bytes_out += (int64_t)n;
			}, sizes);
			if (!ok) return false;
			n_blocks = nb;
			// the tail: what is left of the carry (only when no block was cut), then the end of the device stream, copied home
			const size_t keep_c = used < n_carry ? n_carry - used : 0, d0 = used > n_carry ? used - n_carry : 0, keep_d = n_bytes - d0;
			tail.assign(carry + (n_carry - keep_c), carry + n_carry);
			if (keep_d) {
				if (keep_d >= (size_t)BGZF_IN) throw std::runtime_error("the device sink's tail is a whole block");
				ARX_HIP_CHECK(hipSetDevice(dev));
				ARX_HIP_CHECK(hipMemcpyAsync(h_in[0].p, d_stream + d0, keep_d, hipMemcpyDeviceToHost, st[0]));
				ARX_HIP_CHECK(hipStreamSynchronize(st[0]));
				tail.insert(tail.end(), h_in[0].as<uint8_t>(), h_in[0].as<uint8_t>() + keep_d);
			}
			return true;
		} catch (const std::exception &e) {
			error = e.what();
			return false;
		}
	}
};

} // namespace arx

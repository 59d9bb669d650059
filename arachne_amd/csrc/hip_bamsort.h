// hip_bamsort.h -- dev_bamsort.h on the GPU, and the driver behind arx_bam_sort_append and arx_selftest_bam_sort (arx_bgzf.hip): one BAM file,
// inflated on the device (inflate_launch over the rows of bgzf_walk), its records found, ordered by coordinate and gathered, the stream handed
// to an open writer -- in device memory to a device writer (the path of arx_bam_write_encoded_device), fetched to a host writer.
//
//   k_bs_items<F>    one item of a functor of dev_bamsort.h per thread (probe, walk, verify, tally, fill: an item is a segment; keys, sizes: a
//                    record; gather: one of the BS_GATHER_LANES lanes of a record), started through hip_launch under the functor's name
// The key sort is rocprim::radix_sort_pairs over the key bits that can differ (bs_key_bits), the prefix sums are rocprim's scan.
// The stream, every buffer and rocprim's scratch are owners of hip_res.h (Stream, DevBuf, DevScratch; dev_sort_pairs, dev_two_pass, dev_get); a
// hipMalloc that finds no room (HipOutOfMemory) becomes ARX_E_TOO_LARGE where arx_bgzf.hip catches.
//
// Memory of a sort (all of the file at once): the compressed file (freed once inflated), the inflated stream, the sorted stream, and per record
// 48 bytes of offsets, sizes, keys and values -- about 2.3 times the inflated size at the 300 to 400 bytes of a short-read record.  What does
// not fit is ARX_E_TOO_LARGE: the remedy is a smaller position bucket.  Copy mode holds one slab of whole BGZF blocks at a time.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>
#include <chrono>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/arachne_amd.h"
#include "hip_res.h"
#include "bgzf_walk.h"
#include "dev_bamsort.h"
#include "bam_sink.h"

namespace arx {

void inflate_launch(hipStream_t stream, const uint8_t *d_src, int64_t src_bytes, const InfRow *d_rows, int n_blocks, uint8_t *d_out, int64_t out_bytes, int32_t *d_status,
                    int32_t *d_counts); // arx_bgzf.hip

constexpr int64_t BS_SEG_DEFAULT = 1 << 18;          // seg_bytes of arx_bam_sort_append: the best of 256 KiB, 1 MiB and 4 MiB (profiles/bam_sort/README.md)
constexpr int64_t BS_SLAB_DEFAULT = (int64_t)256 << 20; // inflated bytes of a copy-mode slab where max_bytes is 0
constexpr int BS_N_STATS = 20;
enum { BS_T_READ = 8, BS_T_INFLATE, BS_T_PROBE, BS_T_WALK, BS_T_REPAIR, BS_T_KEYS, BS_T_SORT, BS_T_GATHER, BS_T_WRITE, BS_T_TOTAL };

template <class F> static __global__ void __launch_bounds__(256) k_bs_items(F f, int64_t n)
{
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n) f(i);
}

struct BsTooLarge : std::runtime_error { using std::runtime_error::runtime_error; };

inline double bs_now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// dev_bamsort.h's driver on a stream
struct BsHipDrv {
	hipStream_t st = nullptr;
	bool timed = false;          // wait for every launch and book its time under its phase
	double us[BS_N_STATS] = {0};
	DevScratch tmp;

	static int phase_of(const char *nm)
	{
		if (!strcmp(nm, "bs_probe")) return BS_T_PROBE;
		if (!strcmp(nm, "bs_walk") || !strcmp(nm, "bs_fill")) return BS_T_WALK;
		if (!strcmp(nm, "bs_verify") || !strcmp(nm, "bs_tally")) return BS_T_REPAIR;
		if (!strcmp(nm, "bs_keys")) return BS_T_KEYS;
		if (!strcmp(nm, "bs_sort")) return BS_T_SORT;
		return BS_T_GATHER;
	}
	template <class Fn> void booked(const char *nm, Fn fn)
	{
		if (!timed) { fn(); return; }
		ARX_HIP_CHECK(hipStreamSynchronize(st));
		const double t0 = bs_now_us();
		fn();
		ARX_HIP_CHECK(hipStreamSynchronize(st));
		us[phase_of(nm)] += bs_now_us() - t0;
	}
	template <class F> void items(const char *nm, int64_t n, const F &f)
	{
		if (n <= 0) return;
		const int64_t grid = (n + 255) / 256;
		if (grid > 0x7fffffff) throw BsTooLarge("too many items for one launch: use a smaller position bucket");
		booked(nm, [&]() { hip_launch({"k_bs_items", nm}, k_bs_items<F>, dim3((unsigned)grid), dim3(256), 0, st, f, n); });
	}
	void scan(const int64_t *in, int64_t *out, int64_t n)
	{
		put(&out[0], 0);
		if (n <= 0) return;
		booked("bs_scan", [&]() { dev_two_pass(tmp, "rocprim::inclusive_scan", [&](void *t, size_t &tb) { return rocprim::inclusive_scan(t, tb, in, out + 1, (size_t)n, rocprim::plus<int64_t>(), st); }); });
	}
	int64_t get(const int64_t *p) { return dev_get(p, st); }
	void put(int64_t *p, int64_t v)
	{
		ARX_HIP_CHECK(hipMemcpyAsync(p, &v, 8, hipMemcpyHostToDevice, st));
		ARX_HIP_CHECK(hipStreamSynchronize(st)); // v leaves scope when this returns: the copy has read it by then
	}
	void sort_pairs(const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, int64_t n, int bits) { booked("bs_sort", [&]() { dev_sort_pairs(tmp, kin, kout, vin, vout, (size_t)n, bits, st); }); }
};

constexpr const char *BS_NO_DEVICE = "no such HIP device: the BAM sort runs on the GPU (there is no CPU fallback)"; // select_device's text for the sort's two entries

// the device side of one closed stream: discovery, then (sort) keys, sort and gather.  d_s[0, n): the bytes, records from hdr on
struct BsSorted {
	DevBuf segs, rec_off, mem, out; // out: the sorted records (n - hdr bytes); rec_off: where the records start in d_s
	BsFound found{};
	BsSortMem m{};
	// BS_OK or BS_E_CHAIN; with sort the sorted stream is complete on the stream when this returns
	int run(BsHipDrv &drv, const uint8_t *d_s, int64_t n, int64_t hdr, int64_t seg, int32_t n_ref, bool sort)
	{
		const BsStream t = {d_s, n, hdr, seg, n_ref, 0};
		const int64_t ns = bs_n_seg(t);
		segs.alloc((size_t)bs_seg_words(ns) * 8);
		BsSegs w; w.carve(segs.as<int64_t>(), ns);
		if (bs_discover(drv, t, w, &found) != BS_OK) return BS_E_CHAIN;
		const int64_t N = found.n_records;
		if (N > (int64_t)UINT32_MAX) throw BsTooLarge("more than 2^32 - 1 records in one file: use a smaller position bucket");
		rec_off.alloc((size_t)(N + 1) * 8);
		bs_fill(drv, t, w, found, rec_off.as<int64_t>());
		if (!sort) return BS_OK;
		segs.release();
		mem.alloc((size_t)bs_sort_bytes(N));
		uint8_t *p = mem.as<uint8_t>();
		m.size = (int64_t *)p; p += 8 * N;
		m.out_off = (int64_t *)p; p += 8 * (N + 1);
		m.keys[0] = (uint64_t *)p; p += 8 * N;
		m.keys[1] = (uint64_t *)p; p += 8 * N;
		m.vals[0] = (uint32_t *)p; p += 4 * N;
		m.vals[1] = (uint32_t *)p;
		out.alloc((size_t)(n - hdr));
		bs_sort_gather(drv, d_s, rec_off.as<int64_t>(), N, n_ref, m, out.as<uint8_t>());
		return BS_OK;
	}
};

inline void bs_stats(int64_t *stats, const BsHipDrv &drv, int64_t records, int64_t bytes, int64_t blocks, int64_t segs, int64_t right, int64_t repaired, int64_t rounds, int64_t slabs)
{
	if (!stats) return;
	stats[0] = records; stats[1] = bytes; stats[2] = blocks; stats[3] = segs; stats[4] = right; stats[5] = repaired; stats[6] = rounds; stats[7] = slabs;
	for (int k = 8; k < BS_N_STATS; ++k) stats[k] = (int64_t)drv.us[k];
}

// ---- arx_bam_sort_append
struct BsFile { // the compressed file in host memory and the table of its blocks
	std::vector<uint8_t> raw;
	std::vector<InfRow> rows;     // coff relative to the file, ooff to the inflated stream
	std::vector<int64_t> at;      // where block b starts in the file (n + 1)
	int64_t total = 0;            // inflated bytes
	bool load(const char *path, std::string &err)
	{
		FILE *f = fopen(path, "rb");
		if (!f) { err = std::string("cannot read ") + path; return false; }
		uint8_t buf[1 << 16];
		for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) raw.insert(raw.end(), buf, buf + k);
		const bool bad = ferror(f) != 0;
		fclose(f);
		if (bad) { err = std::string("read error on ") + path; return false; }
		const int64_t n = (int64_t)raw.size();
		for (int64_t o = 0; o < n;) {
			BgzfHeader h;
			if (bgzf_read_header(raw.data() + o, (size_t)(n - o), &h) != 1 || h.block > n - o) { err = std::string(path) + " is not a BGZF file (block " + std::to_string(rows.size()) + " at byte " + std::to_string(o) + ")"; return false; }
			const InfRow r = bgzf_row(raw.data() + o, h, o, total);
			if (r.clen < 0) { err = std::string(path) + ": BGZF block " + std::to_string(rows.size()) + " has a damaged header"; return false; }
			rows.push_back(r); at.push_back(o);
			total += r.isize; o += h.block;
		}
		at.push_back(n);
		if (rows.empty()) { err = std::string(path) + " is empty: not a BAM file"; return false; }
		return true;
	}
	bool host_inflate(size_t b, std::vector<uint8_t> &out) const // one block by zlib, appended (the header's blocks only)
	{
		const InfRow &r = rows[b];
		const size_t o = out.size();
		out.resize(o + (size_t)r.isize);
		z_stream z;
		memset(&z, 0, sizeof z);
		if (inflateInit2(&z, -15) != Z_OK) return false;
		uint8_t none = 0;
		z.next_in = (Bytef *)(raw.data() + r.coff); z.avail_in = (uInt)r.clen; z.next_out = r.isize ? out.data() + o : &none; z.avail_out = (uInt)r.isize;
		const int rc = inflate(&z, Z_FINISH);
		const bool ok = rc == Z_STREAM_END && z.total_out == (uLong)r.isize;
		inflateEnd(&z);
		return ok;
	}
};

// d_src[0, n) of the call's device -- whole records (sort) or a slab of a verified chain (copy) -- -> the writer, ARX_*.  An indexing writer is
// shown the bytes where they lie first (BamSink::admit); then a device writer takes them there (write_dev: the body of
// arx_bam_write_encoded_device behind its own admit), a host writer fetched
template <class WriteDev> int bs_hand_over(BamSink *w, bool device_writer, int device, hipStream_t st, const uint8_t *d_src, int64_t n, int64_t n_records, WriteDev write_dev)
{
	if (n <= 0) return ARX_OK;
	ARX_HIP_CHECK(hipStreamSynchronize(st)); // the stream is complete
	const int rc = w->admit(d_src, n, device);
	if (rc != ARX_OK) return rc;
	if (device_writer) return write_dev(d_src, n, n_records);
	std::vector<uint8_t> h((size_t)n);
	ARX_HIP_CHECK(hipMemcpyAsync(h.data(), d_src, (size_t)n, hipMemcpyDeviceToHost, st));
	ARX_HIP_CHECK(hipStreamSynchronize(st));
	return w->put_raw(h.data(), (size_t)n, n_records) ? ARX_OK : ARX_E_IO;
}

// -> ARX_*; err: the text.  contigs: what the input's header must list
template <class WriteDev> int bs_sort_append(int device, BamSink *w, bool device_writer, WriteDev write_dev, const char *path, int mode, int64_t max_bytes, int32_t n_contigs,
                                             const char *const *names, const int32_t *lens, int64_t *stats, std::string &err)
{
	const bool sort = (mode & 0xff) == ARX_SORT_COORDINATE;
	const double t_begin = bs_now_us();
	BsFile file;
	if (!file.load(path, err)) return ARX_E_IO;
	const int64_t nb = (int64_t)file.rows.size();
	// the header, by zlib from the first blocks
	std::vector<uint8_t> head;
	int64_t hdr = 0;
	int32_t n_ref = 0;
	bool same = true;
	for (size_t b = 0;; ++b) {
		int64_t need = 0;
		same = true;
		const int rc = bs_parse_header(head.data(), (int64_t)head.size(), &need, &n_ref, [&](int32_t i, const char *nm, int64_t l, int32_t len) {
			if (i >= n_contigs || strnlen(nm, (size_t)l) != (size_t)l - 1 || strcmp(nm, names[i]) || len != lens[i]) same = false;
		});
		if (rc == 1) { hdr = need; break; }
		if (rc < 0) { err = std::string(path) + " does not start with a BAM header"; return ARX_E_IO; }
		if ((int64_t)b >= nb) { err = std::string(path) + ": the BAM header is cut short"; return ARX_E_IO; }
		if (!file.host_inflate(b, head)) { err = std::string(path) + ": BGZF block " + std::to_string(b) + " does not inflate"; return ARX_E_IO; }
	}
	if (!same || n_ref != n_contigs) { err = std::string(path) + ": its header does not list the context's contigs (count, names, lengths)"; return ARX_E_ARG; }
	if (hdr > file.total) { err = std::string(path) + ": the BAM header is cut short"; return ARX_E_IO; }
	if (sort && max_bytes > 0 && file.total > max_bytes) {
		err = std::string(path) + " inflates to " + std::to_string(file.total) + " bytes, more than the " + std::to_string(max_bytes) + " allowed: use a smaller position bucket";
		return ARX_E_TOO_LARGE;
	}
	const int64_t slab_max = sort ? file.total : (max_bytes > 0 ? (max_bytes > INF_MAX_OUT ? max_bytes : (int64_t)INF_MAX_OUT) : BS_SLAB_DEFAULT);
	// slabs of whole blocks: [first block, one past the last)
	std::vector<int64_t> cut(1, 0);
	for (int64_t b = 0, in_slab = 0; b < nb; ++b) {
		if (in_slab > 0 && in_slab + file.rows[(size_t)b].isize > slab_max) { cut.push_back(b); in_slab = 0; }
		in_slab += file.rows[(size_t)b].isize;
	}
	cut.push_back(nb);
	const int64_t n_slabs = (int64_t)cut.size() - 1;

	select_device(device, BS_NO_DEVICE);
	Stream st; // the call's own; declared before the buffers, so that it has ended when they are freed
	st.create();
	BsHipDrv drv; drv.st = st; drv.timed = (mode & ARX_SORT_TIMED) != 0;
	drv.us[BS_T_READ] = bs_now_us() - t_begin;
	if (sort) {
		size_t free_b = 0, total_b = 0;
		ARX_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
		// An indexing writer (BamSink::tap) adds nothing to this: before the sorted stream is handed over, the inflated input and the sort's tables are
		// released (below) -- more than the stream's size --, and the index then takes one piece of at most BS_SLAB_DEFAULT bytes of the stream with
		// its carry, 56 bytes per record of the piece and about 100 per run; its window table (8 bytes per 2^min_shift bases) has been there since the open
		const double need = 2.0 * (double)file.total + (double)file.raw.size() + 48.0 * ((double)file.total / 300.0) + 64e6;
		if (need > (double)free_b) {
			err = "sorting " + std::string(path) + " takes about " + std::to_string((int64_t)(need / 1048576.0)) + " MiB of device memory, " + std::to_string(free_b >> 20) + " MiB are free: use a smaller position bucket";
			return ARX_E_TOO_LARGE;
		}
	}
	DevBuf d_comp, d_rows, d_status, d_out, segs;
	BsCarry carry = {hdr, 0, 0, 0, 0, 0};
	uint8_t keep_bytes[BS_SLAB_KEEP] = {0, 0, 0};
	// one slab inflated into d_out behind the `keep` bytes of the one before -> false: a block does not inflate
	auto inflate_slab = [&](int64_t k, int64_t &a, int64_t &b_end) -> bool {
		const double t0 = bs_now_us();
		const int64_t b0 = cut[(size_t)k], b1 = cut[(size_t)k + 1], c0 = file.at[(size_t)b0], c1 = file.at[(size_t)b1];
		a = file.rows[(size_t)b0].ooff; b_end = b1 < nb ? file.rows[(size_t)b1].ooff : file.total;
		const int64_t keep = bs_slab_keep(a), n = keep + b_end - a;
		std::vector<InfRow> rows(file.rows.begin() + b0, file.rows.begin() + b1);
		for (InfRow &r : rows) { r.coff -= c0; r.ooff += keep - a; }
		d_comp.alloc((size_t)(c1 - c0));
		d_rows.alloc(rows.size() * sizeof(InfRow));
		d_status.alloc(4 * (rows.size() + 2));
		d_out.alloc((size_t)n);
		ARX_HIP_CHECK(hipMemcpyAsync(d_comp.p, file.raw.data() + c0, (size_t)(c1 - c0), hipMemcpyHostToDevice, drv.st));
		ARX_HIP_CHECK(hipMemcpyAsync(d_rows.p, rows.data(), rows.size() * sizeof(InfRow), hipMemcpyHostToDevice, drv.st));
		ARX_HIP_CHECK(hipMemsetAsync(d_status.p, 0, 4 * (rows.size() + 2), drv.st));
		if (keep) ARX_HIP_CHECK(hipMemcpyAsync(d_out.p, keep_bytes + (BS_SLAB_KEEP - keep), (size_t)keep, hipMemcpyHostToDevice, drv.st));
		int32_t *counts = d_status.as<int32_t>() + rows.size();
		for (size_t r0 = 0; r0 < rows.size(); r0 += (size_t)1 << 20) { // many blocks a launch
			const size_t nr = rows.size() - r0 < ((size_t)1 << 20) ? rows.size() - r0 : (size_t)1 << 20;
			inflate_launch(drv.st, d_comp.as<uint8_t>(), c1 - c0, d_rows.as<InfRow>() + r0, (int)nr, d_out.as<uint8_t>(), n, d_status.as<int32_t>() + r0, counts);
		}
		int32_t bad[2] = {0, 0};
		ARX_HIP_CHECK(hipMemcpyAsync(bad, counts, 8, hipMemcpyDeviceToHost, drv.st));
		if (n >= BS_SLAB_KEEP) ARX_HIP_CHECK(hipMemcpyAsync(keep_bytes, d_out.as<uint8_t>() + n - BS_SLAB_KEEP, BS_SLAB_KEEP, hipMemcpyDeviceToHost, drv.st));
		ARX_HIP_CHECK(hipStreamSynchronize(drv.st));
		d_comp.release();
		drv.us[BS_T_INFLATE] += bs_now_us() - t0;
		return bad[0] == 0;
	};
	auto write = [&](const uint8_t *d, int64_t n, int64_t n_records) -> int {
		const double t0 = bs_now_us();
		const int rc = bs_hand_over(w, device_writer, device, drv.st, d, n, n_records, write_dev);
		drv.us[BS_T_WRITE] += bs_now_us() - t0;
		return rc;
	};
	auto finish = [&](const BsFound &f) {
		drv.us[BS_T_TOTAL] = bs_now_us() - t_begin;
		bs_stats(stats, drv, f.n_records, file.total, nb, f.n_seg, f.right, f.repaired, f.rounds, n_slabs);
	};
	const char *no_inflate = ": a BGZF block does not inflate", *no_chain = ": the chain of BAM records is broken";
	if (sort) {
		int64_t a = 0, b = 0;
		if (!inflate_slab(0, a, b)) { err = std::string(path) + no_inflate; return ARX_E_IO; }
		BsSorted s;
		if (s.run(drv, d_out.as<uint8_t>(), file.total, hdr, BS_SEG_DEFAULT, n_ref, true) != BS_OK) { err = std::string(path) + no_chain; return ARX_E_IO; }
		if (w->tap) { // room for the index's piece: none of these is read again
			ARX_HIP_CHECK(hipStreamSynchronize(drv.st));
			d_out.release(); s.mem.release(); s.rec_off.release(); s.segs.release();
		}
		const int rc = write(s.out.as<uint8_t>(), file.total - hdr, s.found.n_records);
		if (rc != ARX_OK) { err = w->error; return rc; }
		finish(s.found);
		return ARX_OK;
	}
	// copy: where there are several slabs a first pass only inflates and counts, so that a damaged file appends nothing
	for (int pass = n_slabs > 1 ? 0 : 1; pass < 2; ++pass) {
		carry = BsCarry{hdr, 0, 0, 0, 0, 0};
		for (int64_t k = 0; k < n_slabs; ++k) {
			int64_t a = 0, b = 0;
			if (!inflate_slab(k, a, b)) { err = std::string(path) + no_inflate; return ARX_E_IO; }
			const int64_t keep = bs_slab_keep(a), before = carry.n_records;
			const BsStream t = {d_out.as<uint8_t>(), b - a + keep, bs_slab_entry(a, carry.exit), BS_SEG_DEFAULT, n_ref, 1};
			segs.alloc((size_t)bs_seg_words(bs_n_seg(t)) * 8);
			BsSegs sw; sw.carve(segs.as<int64_t>(), bs_n_seg(t));
			if (bs_count_slab(drv, d_out.as<uint8_t>(), a, b, BS_SEG_DEFAULT, n_ref, sw, carry) != BS_OK || (k + 1 == n_slabs && carry.exit != file.total)) {
				err = std::string(path) + no_chain; return ARX_E_IO;
			}
			const int64_t from = a < hdr ? (hdr < b ? hdr : b) : a; // the header's bytes are not records
			if (pass == 1) {
				const int rc = write(d_out.as<uint8_t>() + keep + (from - a), b - from, carry.n_records - before);
				if (rc != ARX_OK) { err = w->error; return rc; }
			}
		}
	}
	finish(BsFound{carry.n_records, carry.exit, carry.n_seg, carry.right, carry.repaired, carry.rounds});
	return ARX_OK;
}

} // namespace arx

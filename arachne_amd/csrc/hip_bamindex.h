// hip_bamindex.h -- dev_bamindex.h on the GPU, and the drivers behind arx_bam_index and arx_selftest_bam_index (arx_bgzf.hip): one coordinate-
// sorted BAM file, its blocks inflated on the device slab by slab (inflate_launch over the rows of bgzf_walk, as the sort's copy mode), indexed
// there by bi_run, and the .bai written as <path>.tmp and renamed.  arx_bam_index_csi and arx_selftest_bam_index_csi are the same drivers under
// the scheme of a CSI index (bi_csi_scheme), serialised by bi_serialise_csi and written as BGZF by the host sink's own zlib path (BamSink).
// BiWriterTap is the same index built by a writer of what it appends (arx_bam_open_indexed, arx_bam_close_indexed): BiPush behind the sink's tap.
//
//   k_bs_items<F>    hip_bamsort.h's kernel: one item of a functor per thread (bi_tail: the one last record; bi_rec, bi_flag, bi_runs: a record;
//                    bi_head, bi_chunks: a run), started through hip_launch under the functor's name
// The run sort is rocprim::radix_sort_pairs over the key bits that can differ (bi_key_bits), the prefix sums are rocprim's scan.  The stream,
// every buffer and rocprim's scratch are owners of hip_res.h.
//
// Memory: the compressed file in host memory whole (BsFile); on the device the window table (8 bytes per 16384 bases of the contigs; per 2^min_shift
// bases under a CSI scheme) for the whole call, and one slab at a time: its compressed and inflated bytes, the carry in front, 16 bytes per block, 56 per record, about 100 per run.
#pragma once
#include <stdio.h>
#include "hip_bamsort.h"
#include "dev_bamindex.h"

namespace arx {

constexpr int BI_N_STATS = 20;
enum { BI_T_READ = 10, BI_T_INFLATE, BI_T_DISCOVER, BI_T_RECORDS, BI_T_RUNS, BI_T_WRITE, BI_T_TOTAL };
constexpr const char *BI_NO_DEVICE = "no such HIP device: the BAM index is built on the GPU (there is no CPU fallback)";

// dev_bamindex.h's driver on a stream
struct BiHipDrv {
	typedef DevBuf Buf;
	hipStream_t st = nullptr;
	bool timed = false; // wait for every launch and book its time under its phase
	double us[BI_N_STATS] = {0};
	DevScratch tmp;

	static int phase_of(const char *nm)
	{
		if (!strncmp(nm, "bs_", 3)) return BI_T_DISCOVER;
		if (!strcmp(nm, "bi_tail") || !strcmp(nm, "bi_rec") || !strcmp(nm, "bi_flag")) return BI_T_RECORDS;
		return BI_T_RUNS;
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
		if (grid > 0x7fffffff) throw BsTooLarge("too many items for one launch: use a smaller max_bytes");
		booked(nm, [&]() { hip_launch({"k_bs_items", nm}, k_bs_items<F>, dim3((unsigned)grid), dim3(256), 0, st, f, n); });
	}
	void scan(const int64_t *in, int64_t *out, int64_t n, const char *nm = "bs_scan")
	{
		put(&out[0], 0);
		if (n <= 0) return;
		booked(nm, [&]() { dev_two_pass(tmp, "rocprim::inclusive_scan", [&](void *t, size_t &tb) { return rocprim::inclusive_scan(t, tb, in, out + 1, (size_t)n, rocprim::plus<int64_t>(), st); }); });
	}
	int64_t get(const int64_t *p) { return dev_get(p, st); }
	void put(int64_t *p, int64_t v) { upload(p, &v, 8); }
	void sort_pairs(const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, int64_t n, int bits) { booked("bi_sort", [&]() { dev_sort_pairs(tmp, kin, kout, vin, vout, (size_t)n, bits, st); }); }
	void upload(void *d, const void *h, size_t n) // h may leave scope when this returns: the copy has read it by then
	{
		if (!n) return;
		ARX_HIP_CHECK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, st));
		ARX_HIP_CHECK(hipStreamSynchronize(st));
	}
	void fetch(void *h, const void *d, size_t n)
	{
		if (!n) return;
		ARX_HIP_CHECK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, st));
		ARX_HIP_CHECK(hipStreamSynchronize(st));
	}
	void copy(void *d, const void *s, size_t n) { if (n) ARX_HIP_CHECK(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, st)); }
	void fill(void *d, int byte, size_t n) { if (n) ARX_HIP_CHECK(hipMemsetAsync(d, byte, n, st)); }
};

inline void bi_stats(int64_t *stats, const BiHipDrv &drv, const BiIndex &ix, int64_t bytes, int64_t blocks)
{
	if (!stats) return;
	stats[0] = ix.n_records; stats[1] = bytes; stats[2] = blocks; stats[3] = ix.n_slabs; stats[4] = ix.n_runs; stats[5] = ix.n_chunks; stats[6] = ix.n_bins;
	stats[7] = ix.n_lin; stats[8] = ix.n_no_coor;
	for (int k = BI_T_READ; k <= BI_T_TOTAL; ++k) stats[k] = (int64_t)drv.us[k];
}

inline std::string bi_long_text(int32_t i, int64_t len)
{
	return "contig " + std::to_string(i) + " has " + std::to_string(len) + " bases, more than the 2^29 a BAI index can hold (arx_bam_index_csi writes the CSI index of such a file)";
}
// under a CSI scheme: [7] the depth chosen in place of the linear entries, which a .csi does not hold, and [17] min_shift as used
inline void bi_stats_csi(int64_t *stats, const BiScheme &sc)
{
	if (!stats) return;
	stats[7] = sc.depth; stats[17] = sc.min_shift;
}

// a slab of the selftest: the stream lies in device memory already
struct BiMemSrc {
	BiHipDrv &drv; const uint8_t *d_stream; const BiBlocks &B;
	bool load(int64_t k, uint8_t *dst, int64_t n) { drv.copy(dst, d_stream + B.cut_o[(size_t)k], (size_t)n); return true; }
};
// a slab of a file: its blocks uploaded and inflated where the buffer wants them
struct BiFileSrc {
	BiHipDrv &drv; const BsFile &file; const BiBlocks &B;
	DevBuf d_comp, d_rows, d_status;
	bool load(int64_t k, uint8_t *dst, int64_t n)
	{
		const double t0 = bs_now_us();
		const int64_t b0 = B.cut_b[(size_t)k], b1 = B.cut_b[(size_t)k + 1], c0 = file.at[(size_t)b0], c1 = file.at[(size_t)b1], a = B.cut_o[(size_t)k];
		std::vector<InfRow> rows(file.rows.begin() + b0, file.rows.begin() + b1);
		for (InfRow &r : rows) { r.coff -= c0; r.ooff -= a; }
		d_comp.alloc((size_t)(c1 - c0));
		d_rows.alloc(rows.size() * sizeof(InfRow));
		d_status.alloc(4 * (rows.size() + 2));
		ARX_HIP_CHECK(hipMemcpyAsync(d_comp.p, file.raw.data() + c0, (size_t)(c1 - c0), hipMemcpyHostToDevice, drv.st));
		ARX_HIP_CHECK(hipMemcpyAsync(d_rows.p, rows.data(), rows.size() * sizeof(InfRow), hipMemcpyHostToDevice, drv.st));
		ARX_HIP_CHECK(hipMemsetAsync(d_status.p, 0, 4 * (rows.size() + 2), drv.st));
		int32_t *counts = d_status.as<int32_t>() + rows.size();
		for (size_t r0 = 0; r0 < rows.size(); r0 += (size_t)1 << 20) { // many blocks a launch
			const size_t nr = rows.size() - r0 < ((size_t)1 << 20) ? rows.size() - r0 : (size_t)1 << 20;
			inflate_launch(drv.st, d_comp.as<uint8_t>(), c1 - c0, d_rows.as<InfRow>() + r0, (int)nr, dst, n, d_status.as<int32_t>() + r0, counts);
		}
		int32_t bad[2] = {0, 0};
		ARX_HIP_CHECK(hipMemcpyAsync(bad, counts, 8, hipMemcpyDeviceToHost, drv.st));
		ARX_HIP_CHECK(hipStreamSynchronize(drv.st)); // rows and bad are the host's
		d_comp.release();
		drv.us[BI_T_INFLATE] += bs_now_us() - t0;
		return bad[0] == 0;
	}
};

// bi_run's result as one of ARX_*, with the text
inline int bi_result(int rc, const BiIndex &ix, const std::string &what, std::string &err)
{
	if (rc == BI_OK) return ARX_OK;
	if (rc == BI_E_RULE) {
		err = what + ": " + bi_rule_text(ix.err);
		return (ix.err & 0xff) == BI_R_FIELDS ? ARX_E_IO : ARX_E_ARG;
	}
	err = what + (rc == BI_E_INFLATE ? ": a BGZF block does not inflate" : ": the chain of BAM records is broken");
	return ARX_E_IO;
}

// the index's bytes as <final_path>.tmp, renamed at the end; bgzf: as BGZF blocks of at most 65,280 input bytes with the EOF block last, compressed
// by the host sink's zlib path
inline bool bi_write_file(const std::vector<uint8_t> &out, const std::string &final_path, bool bgzf, std::string &err)
{
	const std::string tmp_path = final_path + ".tmp";
	FILE *f = fopen(tmp_path.c_str(), "wb");
	if (!f) { err = "cannot write " + tmp_path; return false; }
	bool done;
	if (bgzf) {
		BamSink sink;
		sink.f = f;
		sink.pending = out;
		done = sink.close(); // every block of what is pending, the EOF block, fclose
	} else {
		const bool wrote = fwrite(out.data(), 1, out.size(), f) == out.size();
		done = (fclose(f) == 0) && wrote;
	}
	if (!done || rename(tmp_path.c_str(), final_path.c_str()) != 0) {
		remove(tmp_path.c_str());
		err = "cannot write " + final_path;
		return false;
	}
	return true;
}

// ---- the index a writer builds of what it is handed (arx_bam_open_indexed): BiPush behind the sink's tap (bam_sink.h: StreamTap).  Bytes that lie
// in the memory of the writer's device are fed where they lie; host bytes go up in pieces of at most BI_UPLOAD.  The index is all or nothing: after an
// append it refused, or an error of its own (which refuses nothing), the tap lets everything pass and the close writes no index
constexpr int64_t BI_UPLOAD = (int64_t)64 << 20;
struct BiWriterTap : StreamTap {
	int device = 0;
	bool csi = false, live = true;
	int lost = ARX_E_ARG;        // what the close returns once the index is lost
	std::string index_path, why; // why: what lost the index
	Stream st;                   // declared before the buffers, so that it has ended when they are freed
	BiHipDrv drv;
	BiPush<BiHipDrv> push;
	DevBuf stage;
	int64_t header = 0;
	double us_index = 0;

	void begin(int device_, const BiScheme &sc, bool csi_, const std::string &path, int32_t n_ref, const int32_t *ref_len, int64_t H)
	{
		device = device_; csi = csi_; index_path = path; header = H;
		select_device(device, BI_NO_DEVICE);
		st.create();
		drv.st = st;
		push.begin(drv, n_ref, ref_len, sc, H, BS_SEG_DEFAULT, BS_SLAB_DEFAULT);
	}
	~BiWriterTap() override { (void)hipSetDevice(device); } // (the members are this device's)

	int take(const uint8_t *p, int64_t n, int dev, std::string &error) override
	{
		if (!live) return ARX_OK;
		if (dev >= 0 && dev != device) {
			error = "the bytes lie on device " + std::to_string(dev) + ", the writer's index is built on device " + std::to_string(device) + ": append through a context of the writer's device";
			return ARX_E_ARG; // nothing was fed: the index goes on
		}
		const double t0 = bs_now_us();
		int rc = BI_OK;
		try {
			select_device(device, BI_NO_DEVICE);
			if (dev >= 0) rc = push.feed(drv, p, n);
			for (int64_t o = 0; dev < 0 && o < n && rc == BI_OK;) {
				const int64_t len = n - o < BI_UPLOAD ? n - o : BI_UPLOAD;
				stage.alloc((size_t)len);
				drv.upload(stage.p, p + o, (size_t)len);
				rc = push.feed(drv, stage.as<uint8_t>(), len);
				o += len;
			}
			stage.release();
			ARX_HIP_CHECK(hipStreamSynchronize(st));
		} catch (const std::exception &e) { // the index's own trouble (device memory, say) keeps no append out: the BAM goes on, the close reports it
			live = false; lost = ARX_E_DEVICE;
			why = e.what();
			return ARX_OK;
		}
		us_index += bs_now_us() - t0;
		if (rc == BI_OK) return ARX_OK;
		live = false;
		const int code = bi_result(rc, push.ix, "the append was refused, nothing of it was written", error);
		why = rc == BI_E_RULE ? bi_rule_text(push.ix.err) : "the chain of BAM records is broken";
		return code;
	}

	int finish(const std::vector<int64_t> &block_at, bool bam_ok, int64_t *stats, std::string &error) override
	{
		if (!bam_ok) return ARX_OK; // the close's own error stands
		if (!live) { error = "the BAM is complete, the index was not written: " + why; return lost; }
		const double t0 = bs_now_us();
		select_device(device, BI_NO_DEVICE);
		const int64_t nb = push.n_blocks();
		if ((int64_t)block_at.size() != nb + 1) { error = "the BAM is complete, the index was not written: the sink recorded " + std::to_string(block_at.size()) + " blocks where its layout has " + std::to_string(nb + 1); return ARX_E_DEVICE; }
		if (block_at.back() >= BI_MAX_AT) { error = "the BAM is complete, the index was not written: the file is 2^48 bytes or longer, a virtual offset cannot address it"; return ARX_E_ARG; }
		if (push.finish(drv, block_at.data()) != BI_OK) { error = "the BAM is complete, the index was not written: the record stream ends inside a record"; return ARX_E_IO; }
		const double t_w = bs_now_us();
		const std::vector<uint8_t> out = csi ? bi_serialise_csi(push.ix) : bi_serialise(push.ix);
		if (!bi_write_file(out, index_path, csi, error)) return ARX_E_IO;
		drv.us[BI_T_WRITE] = bs_now_us() - t_w;
		drv.us[BI_T_TOTAL] = us_index + (bs_now_us() - t0);
		bi_stats(stats, drv, push.ix, header + push.total, nb);
		if (csi) bi_stats_csi(stats, push.ix.sc);
		return ARX_OK;
	}
};

// -> ARX_*; err: the text.  csi_shift: 0 for the .bai, else the min_shift of the .csi (bi_csi_shift's result)
inline int bi_index_file(int device, const char *path, const char *bai_path, int64_t max_bytes, bool timed, int64_t *stats, std::string &err, int32_t csi_shift = 0)
{
	const double t_begin = bs_now_us();
	BsFile file;
	if (!file.load(path, err)) return ARX_E_IO;
	const int64_t nb = (int64_t)file.rows.size();
	// the header, by zlib from the first blocks
	std::vector<uint8_t> head;
	std::vector<int32_t> ref_len;
	int64_t hdr = 0;
	int32_t n_ref = 0;
	for (size_t b = 0;; ++b) {
		int64_t need = 0;
		ref_len.clear();
		const int rc = bs_parse_header(head.data(), (int64_t)head.size(), &need, &n_ref, [&](int32_t, const char *, int64_t, int32_t len) { ref_len.push_back(len); });
		if (rc == 1) { hdr = need; break; }
		if (rc < 0) { err = std::string(path) + " does not start with a BAM header"; return ARX_E_IO; }
		if ((int64_t)b >= nb) { err = std::string(path) + ": the BAM header is cut short"; return ARX_E_IO; }
		if (!file.host_inflate(b, head)) { err = std::string(path) + ": BGZF block " + std::to_string(b) + " does not inflate"; return ARX_E_IO; }
	}
	if (hdr > file.total) { err = std::string(path) + ": the BAM header is cut short"; return ARX_E_IO; }
	const bool csi = csi_shift != 0;
	const BiScheme sc = csi ? bi_csi_scheme(csi_shift, n_ref, ref_len.data()) : BI_BAI;
	const int32_t too_long = csi ? -1 : bi_long_contig(n_ref, ref_len.data());
	if (too_long >= 0) { err = std::string(path) + ": " + bi_long_text(too_long, ref_len[(size_t)too_long]); return ARX_E_ARG; }
	std::vector<int32_t> isize((size_t)nb);
	for (int64_t b = 0; b < nb; ++b) isize[(size_t)b] = file.rows[(size_t)b].isize;
	BiBlocks B;
	if (!B.build(nb, file.at.data(), isize.data(), max_bytes > 0 ? max_bytes : BS_SLAB_DEFAULT)) {
		err = std::string(path) + " is 2^48 bytes or longer: a virtual offset cannot address it"; return ARX_E_ARG;
	}

	select_device(device, BI_NO_DEVICE);
	Stream st; // the call's own; declared before the buffers, so that it has ended when they are freed
	st.create();
	BiHipDrv drv; drv.st = st; drv.timed = timed;
	drv.us[BI_T_READ] = bs_now_us() - t_begin;
	BiIndex ix;
	{
		BiFileSrc src{drv, file, B};
		const int rc = bi_result(bi_run(drv, src, B, hdr, n_ref, ref_len.data(), BS_SEG_DEFAULT, ix, sc), ix, path, err);
		if (rc != ARX_OK) return rc;
	}
	const double t_w = bs_now_us();
	const std::vector<uint8_t> out = csi ? bi_serialise_csi(ix) : bi_serialise(ix);
	const std::string final_path = bai_path ? std::string(bai_path) : std::string(path) + (csi ? ".csi" : ".bai");
	if (!bi_write_file(out, final_path, csi, err)) return ARX_E_IO;
	drv.us[BI_T_WRITE] = bs_now_us() - t_w;
	drv.us[BI_T_TOTAL] = bs_now_us() - t_begin;
	bi_stats(stats, drv, ix, file.total, nb);
	if (csi) bi_stats_csi(stats, sc);
	return ARX_OK;
}

} // namespace arx

// arx_bgzf.hip -- the device BAM sink (include/arachne_amd.h: arx_bam_open_device, arx_bam_write_encoded_device, arx_selftest_bgzf): BamSink (bam_sink.h) with the compressor of
// hip_bgzf.h behind its seam.  Its own unit: the kernels of dev_bgzf.h compile next to the pipeline's.  The mirror image lives here too: the
// inflate kernel of hip_inflate.h (arx_selftest_inflate; the device feeder starts it through inflate_launch).  And what needs both: the coordinate
// sort of a BAM file into an open writer (arx_bam_open_ex, arx_bam_sort_append, arx_selftest_bam_sort: dev_bamsort.h, hip_bamsort.h), and the sort
// of a FASTQ file pair by barcode (arx_fastq_sort, arx_selftest_fastq_sort: dev_fqsort.h, hip_fqsort.h) with the header standardization in front of it (arx_fastq_standardize,
// arx_selftest_fastq_standardize: dev_fqstd.h, hip_fqstd.h) and the two fused into one call (arx_fastq_prepare, arx_selftest_fastq_prepare: dev_fqprep.h, hip_fqprep.h), and the .bai of a coordinate-sorted
// BAM file and its .csi (arx_bam_index, arx_bam_index_csi and their self-tests: dev_bamindex.h, hip_bamindex.h).  The FASTQ calls' readers also
// serve the index build that reads and packs its FASTA on the device (arx_index_build_ex, arx_selftest_fasta_pack: dev_fapack.h, hip_fapack.h).
#include <map>
#include <memory>
#include <mutex>
#include "../../include/arachne_amd.h"
#include "hip_bgzf.h"
#include "hip_inflate.h"
#include "hip_gunzip.h"
#include "hip_bamsort.h"
#include "hip_fqsort.h"
#include "hip_fqstd.h"
#include "hip_fqprep.h"
#include "hip_fapack.h"
#include "hip_bamindex.h"

namespace arx {

// One compressor per device, made by the first writer (or self-test) that asks for it and kept until the process ends: its streams, staging and
// device buffers are sized once and reused by every later writer (the reference layout keeps one writer per position bucket open; e2e.run opens
// writers run after run).  The map itself is never destroyed, so that no HIP call runs from a static destructor.
static std::shared_ptr<DeviceBgzf> shared_device_bgzf(int device)
{
	static std::mutex mu;
	static std::map<int, std::shared_ptr<DeviceBgzf> > *live = new std::map<int, std::shared_ptr<DeviceBgzf> >();
	std::lock_guard<std::mutex> lock(mu);
	std::shared_ptr<DeviceBgzf> &p = (*live)[device];
	if (!p) {
		std::shared_ptr<DeviceBgzf> z = std::make_shared<DeviceBgzf>();
		z->init(device);
		p = z;
	}
	return p;
}

void inflate_launch(hipStream_t stream, const uint8_t *d_src, int64_t src_bytes, const InfRow *d_rows, int n_blocks, uint8_t *d_out, int64_t out_bytes, int32_t *d_status,
                    int32_t *d_counts)
{
	if (n_blocks <= 0) return;
	// per device and cheap; set on every launch rather than remembered per device
	ARX_HIP_CHECK(hipFuncSetAttribute((const void *)k_bgzf_inflate, hipFuncAttributeMaxDynamicSharedMemorySize, INF_LDS_BYTES));
	hip_launch("k_bgzf_inflate", k_bgzf_inflate, dim3(n_blocks), dim3(INF_LANES), INF_LDS_BYTES, stream, d_src, src_bytes, d_rows, n_blocks, d_out, out_bytes, d_status, d_counts);
}

// The device feeder's backend for a gzip file (device_feeder.h declares these and calls them from arx_api.hip): a GzHip on a stream of its own,
// so that R1's and R2's launches run side by side.  The calling thread's device is the feeder's
struct GzFeedDev {
	Stream st; // declared before the backend: its buffers are freed first, behind the wait of gz_feed_close
	GzHip dev;
};
GzFeedDev *gz_feed_open()
{
	std::unique_ptr<GzFeedDev> d(new GzFeedDev());
	d->st.create();
	d->dev.init(d->st);
	return d.release();
}
void gz_feed_close(GzFeedDev *d)
{
	if (!d) return;
	(void)hipStreamSynchronize(d->st);
	delete d;
}
void gz_feed_decode_begin(GzFeedDev *d, const uint8_t *src, int clen, int start_bit, const uint8_t *window, int have, int chunk_bytes, int expand)
{
	d->dev.decode_begin(src, clen, start_bit, window, have, chunk_bytes, expand);
}
void gz_feed_decode_end(GzFeedDev *d, GzLaunch &L) { d->dev.decode_end(L); }
void gz_feed_resolve_begin(GzFeedDev *d, GzLaunch &L, uint8_t *text, hipStream_t after) { d->dev.resolve_begin(L, text, after); }
void gz_feed_resolve_end(GzFeedDev *d, GzLaunch &L) { d->dev.resolve_end(L); }
// a piece of the host's to its place behind the carry: behind what the feeder's stream holds for the window, and waited for
void gz_feed_upload(GzFeedDev *d, uint8_t *dst, const uint8_t *host, size_t bytes, hipStream_t after)
{
	if (!bytes) return;
	Event made(hipEventDisableTiming);
	ARX_HIP_CHECK(hipEventRecord(made, after));
	ARX_HIP_CHECK(hipStreamWaitEvent(d->st, made, 0));
	d->dev.upload(dst, host, bytes);
}

} // namespace arx

extern "C" int arx_bam_open_device(arx_ctx *ctx, const char *path, int32_t n_contigs, const char *const *names, const int32_t *lens, const char *extra_header,
                                   int32_t threads, arx_bam **out, char *msg, int32_t msg_cap)
{
	auto say = [&](const char *m) { if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "%s", m); };
	if (out) *out = nullptr;
	if (!ctx) { say("arx_bam_open_device: null context"); return ARX_E_ARG; }
	if (!out || !path || n_contigs < 0 || (n_contigs > 0 && (!names || !lens))) { say("arx_bam_open_device: null argument"); return ARX_E_ARG; }
	arx::BamSink *w = nullptr;
	try {
		w = new arx::BamSink();
		w->comp = arx::shared_device_bgzf(arx_ctx_device(ctx));
		if (!w->open(path, n_contigs, names, lens, extra_header, threads, 1)) {
			const bool io = !w->f;
			say(w->error.c_str());
			delete w;
			return io ? ARX_E_IO : ARX_E_DEVICE;
		}
	} catch (const std::exception &e) {
		say(e.what());
		delete w;
		return ARX_E_DEVICE;
	}
	*out = (arx_bam *)w;
	return ARX_OK;
}

// d_stream[0, n_bytes) of the compressor's device, behind the writer's carry, through the device sink.  admitted: an indexing writer has seen
// these bytes already (bs_hand_over); otherwise it is shown them here, before anything is appended
static int bam_write_device(arx::BamSink *w, const uint8_t *d_stream, int64_t n_bytes, int64_t n_records, bool admitted)
{
	if (!w) return ARX_E_ARG;
	arx::DeviceBgzf *z = dynamic_cast<arx::DeviceBgzf *>(w->comp.get());
	if (!z) { w->error = "arx_bam_write_encoded_device on a writer of arx_bam_open: only arx_bam_open_device's writers take a device stream"; return ARX_E_ARG; }
	if (n_bytes < 0 || n_records < 0 || (n_bytes > 0 && !d_stream)) { w->error = "arx_bam_write_encoded_device: bad arguments"; return ARX_E_ARG; }
	if (n_bytes == 0) { if (n_records) { w->error = "arx_bam_write_encoded_device: records without bytes"; return ARX_E_ARG; } return ARX_OK; }
	try {
		if (!admitted) {
			const int rc = w->admit(d_stream, n_bytes, z->dev);
			if (rc != ARX_OK) return rc;
		}
		// a write on the host side may have left whole blocks pending only if its flush failed; the carry handed on is always short of a block
		if (!w->flush(false)) return ARX_E_IO;
		std::vector<uint8_t> tail;
		std::vector<int64_t> sizes;
		size_t nb = 0;
		const int64_t from = w->bytes_out;
		if (!z->run_device(w->pending.data(), w->pending.size(), d_stream, (size_t)n_bytes, w->f, w->bytes_out, nb, tail, w->error, w->record_blocks ? &sizes : nullptr)) return ARX_E_IO;
		if (w->record_blocks) {
			if (sizes.size() != nb) { w->error = "the compressor reported the sizes of " + std::to_string(sizes.size()) + " blocks, not " + std::to_string(nb); return ARX_E_IO; }
			w->note_blocks(sizes, from);
		}
		w->n_blocks += (int64_t)nb; w->bytes_in += (int64_t)(nb * arx::BamSink::BLOCK_IN);
		w->pending.swap(tail);
		w->n_records += n_records;
	} catch (const std::exception &e) {
		w->error = e.what();
		return ARX_E_IO;
	}
	return ARX_OK;
}
extern "C" int arx_bam_write_encoded_device(arx_bam *h, const uint8_t *d_stream, int64_t n_bytes, int64_t n_records)
{
	return bam_write_device((arx::BamSink *)h, d_stream, n_bytes, n_records, false);
}

extern "C" int arx_selftest_bgzf(int32_t device, const uint8_t *src, int64_t n, uint8_t *out, int64_t cap, int64_t *out_len, int64_t *stats)
{
	if (n < 0 || cap < 0 || !out_len || (n > 0 && (!src || !out))) return ARX_E_ARG;
	*out_len = 0;
	if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
	if (n == 0) return ARX_OK;
	try {
		std::shared_ptr<arx::DeviceBgzf> zp = arx::shared_device_bgzf(device);
		arx::DeviceBgzf &z = *zp;
		std::lock_guard<std::mutex> lock(z.mu); // a flush at a time; the counts of the forms below are this call's
		const int64_t before[3] = {z.n_form[0], z.n_form[1], z.n_form[2]};
		int64_t at = 0;
		bool fits = true;
		z.compress(src, (size_t)n, [&](const uint8_t *p, size_t bytes) {
			if (fits && at + (int64_t)bytes <= cap) { memcpy(out + at, p, bytes); at += (int64_t)bytes; } else fits = false;
		});
		if (!fits) return ARX_E_ARG;
		*out_len = at;
		if (stats) { stats[0] = (n + arx::BGZF_IN - 1) / arx::BGZF_IN; stats[1] = z.n_form[0] - before[0]; stats[2] = z.n_form[1] - before[1]; stats[3] = z.n_form[2] - before[2]; }
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
	return ARX_OK;
}

extern "C" int arx_selftest_inflate(int32_t device, const uint8_t *src, int64_t n, uint8_t *out, int64_t cap, int64_t *out_len, int32_t *status, int32_t status_cap,
                                    int64_t *stats)
{
	static_assert(ARX_INFLATE_CRC_MISMATCH == arx::INF_CRC_MISMATCH && ARX_INFLATE_BAD_HEADER == arx::INF_BAD_HEADER, "the public statuses are dev_inflate.h's");
	if (n < 0 || cap < 0 || status_cap < 0 || !out_len || (n > 0 && (!src || !status)) || (cap > 0 && !out)) return ARX_E_ARG;
	*out_len = 0;
	if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
	if (n == 0) return ARX_OK;
	int64_t total = 0;
	const int64_t nb = arx::bgzf_walk(src, n, nullptr, 0, &total);
	if (nb < 0 || nb > status_cap || nb > INT32_MAX || total > cap) return ARX_E_ARG;
	std::vector<arx::InfRow> rows((size_t)nb);
	arx::bgzf_walk(src, n, rows.data(), nb, &total);
	int rc = ARX_OK;
	try {
		arx::select_device(device, "no such HIP device");
		arx::DevBuf src_buf((size_t)n), out_buf((size_t)total), rows_buf(sizeof(arx::InfRow) * (size_t)nb), status_buf(4 * ((size_t)nb + 2));
		uint8_t *d_src = src_buf.as<uint8_t>(), *d_out = out_buf.as<uint8_t>();
		arx::InfRow *d_rows = rows_buf.as<arx::InfRow>();
		int32_t *d_status = status_buf.as<int32_t>(); // nb statuses, then the two counts
		ARX_HIP_CHECK(hipMemcpy(d_src, src, (size_t)n, hipMemcpyHostToDevice));
		ARX_HIP_CHECK(hipMemcpy(d_rows, rows.data(), sizeof(arx::InfRow) * (size_t)nb, hipMemcpyHostToDevice));
		if (total) ARX_HIP_CHECK(hipMemcpy(d_out, out, (size_t)total, hipMemcpyHostToDevice)); // what a bad block leaves alone comes back as it was
		ARX_HIP_CHECK(hipMemset(d_status, 0, 4 * ((size_t)nb + 2)));
		arx::inflate_launch(nullptr, d_src, n, d_rows, (int)nb, d_out, total, d_status, d_status + nb);
		ARX_HIP_CHECK(hipDeviceSynchronize());
		int32_t counts[2];
		ARX_HIP_CHECK(hipMemcpy(status, d_status, 4 * (size_t)nb, hipMemcpyDeviceToHost));
		ARX_HIP_CHECK(hipMemcpy(counts, d_status + nb, 8, hipMemcpyDeviceToHost));
		if (total) ARX_HIP_CHECK(hipMemcpy(out, d_out, (size_t)total, hipMemcpyDeviceToHost));
		int64_t good = 0, n_bad = 0;
		bool all = true;
		for (int64_t b = 0; b < nb; ++b) {
			if (status[b] != arx::INF_OK) { all = false; ++n_bad; }
			if (all) good += rows[(size_t)b].isize;
		}
		if (n_bad != counts[0]) rc = ARX_E_DEVICE; // the count the feeder relies on is the statuses'
		else rc = all ? ARX_OK : ARX_E_IO;
		*out_len = good;
		if (stats) { stats[0] = nb; stats[1] = n; stats[2] = total; stats[3] = counts[1]; }
	} catch (const std::exception &) {
		rc = ARX_E_DEVICE;
	}
	return rc;
}

// ---- the chunked inflate of a plain gzip file (dev_gunzip.h, hip_gunzip.h, gunzip_host.h)
extern "C" int arx_selftest_gunzip(int32_t device, const uint8_t *src, int64_t n, int64_t chunk_bytes, int64_t slab_bytes, int32_t expand, uint8_t *out, int64_t cap,
                                   int64_t *out_len, int64_t *stats)
{
	static_assert(ARX_GUNZIP_N_STATS == arx::GZ_N_STATS && ARX_GUNZIP_FB_CUT_SHORT == arx::GZ_FB_CUT_SHORT, "the public statistics are gunzip_host.h's");
	const int64_t chunk = chunk_bytes ? chunk_bytes : arx::GZ_CHUNK_DEFAULT, slab = slab_bytes ? slab_bytes : arx::GZ_SLAB_DEFAULT < 2 * chunk ? 2 * chunk : arx::GZ_SLAB_DEFAULT > arx::GZ_MAX_CHUNKS * chunk ? arx::GZ_MAX_CHUNKS * chunk : arx::GZ_SLAB_DEFAULT;
	const int32_t ex = expand ? expand : arx::GZ_EXPAND_DEFAULT;
	if (n < 0 || cap < 0 || !out_len || (n > 0 && !src) || (cap > 0 && !out) || chunk_bytes < 0 || slab_bytes < 0 || chunk < arx::GZ_MIN_CHUNK || chunk > arx::GZ_MAX_SLAB / 2 ||
	    slab < 2 * chunk || slab > arx::GZ_MAX_SLAB || slab > arx::GZ_MAX_CHUNKS * chunk || ex < 1 || ex > arx::GZ_MAX_EXPAND || slab * ex > arx::GZ_MAX_SYMBOLS)
		return ARX_E_ARG;
	*out_len = 0;
	if (stats) for (int k = 0; k < arx::GZ_N_STATS; ++k) stats[k] = 0;
	try {
		arx::select_device(device, "no such HIP device");
		arx::Stream st; // declared before the buffers, so that it has ended when they are freed
		st.create();
		arx::GzHip dev;
		dev.init(st);
		arx::GzMemSource in(src, n);
		arx::GzReader<arx::GzHip> r(dev, in, chunk, slab, ex);
		r.can_rewind = true;
		arx::DevBuf d_text; // a piece at its place in device memory, then home
		std::vector<uint8_t> text;
		for (;;) {
			const int64_t k = r.next();
			if (k == arx::GZ_END) break;
			if (k == arx::GZ_ERROR) return ARX_E_IO;
			if (k == arx::GZ_REWIND) { text.resize((size_t)r.rewind_to); continue; }
			if (!d_text.p || d_text.bytes < (size_t)k) d_text.alloc((size_t)k);
			r.place(d_text.as<uint8_t>());
			const size_t at = text.size();
			text.resize(at + (size_t)k);
			ARX_HIP_CHECK(hipMemcpyAsync(text.data() + at, d_text.p, (size_t)k, hipMemcpyDeviceToHost, st));
			ARX_HIP_CHECK(hipStreamSynchronize(st));
		}
		if ((int64_t)text.size() > cap) return ARX_E_ARG;
		if (!text.empty()) memcpy(out, text.data(), text.size());
		*out_len = (int64_t)text.size();
		if (stats) for (int k = 0; k < arx::GZ_N_STATS; ++k) stats[k] = r.stats[k];
	} catch (const arx::HipOutOfMemory &) {
		return ARX_E_TOO_LARGE;
	} catch (const std::bad_alloc &) {
		return ARX_E_TOO_LARGE;
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
	return ARX_OK;
}

extern "C" int arx_fastq_gunzip_counters(int64_t *counters, int32_t reset)
{
	static_assert(ARX_GUNZIP_N_COUNTERS == arx::GZC_N, "the public counters are hip_fqsort.h's");
	if (!counters) return ARX_E_ARG;
	for (int k = 0; k < arx::GZC_N; ++k) counters[k] = reset ? arx::gz_counters()[k].exchange(0) : arx::gz_counters()[k].load();
	return ARX_OK;
}

// ---- the coordinate sort of a BAM file into an open writer (dev_bamsort.h, hip_bamsort.h)
extern "C" int arx_bam_open_ex(arx_ctx *ctx, const char *path, int32_t n_contigs, const char *const *names, const int32_t *lens, const char *extra_header, int32_t threads,
                               int32_t level, int32_t flags, arx_bam **out, char *msg, int32_t msg_cap)
{
	auto say = [&](const char *m) { if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "%s", m); };
	if (out) *out = nullptr;
	if (!out || !path || n_contigs < 0 || (n_contigs > 0 && (!names || !lens))) { say("arx_bam_open_ex: null argument"); return ARX_E_ARG; }
	if (flags & ~ARX_BAM_COORDINATE) { say("arx_bam_open_ex: unknown flag bits"); return ARX_E_ARG; }
	arx::BamSink *w = nullptr;
	try {
		w = new arx::BamSink();
		w->coordinate = (flags & ARX_BAM_COORDINATE) != 0;
		if (ctx) w->comp = arx::shared_device_bgzf(arx_ctx_device(ctx));
		if (!w->open(path, n_contigs, names, lens, extra_header, threads, ctx ? 1 : level)) {
			const bool io = !ctx || !w->f;
			say(w->error.c_str());
			delete w;
			return io ? ARX_E_IO : ARX_E_DEVICE;
		}
	} catch (const std::exception &e) {
		say(e.what());
		delete w;
		return ctx ? ARX_E_DEVICE : ARX_E_IO;
	}
	*out = (arx_bam *)w;
	return ARX_OK;
}

// ---- the writer that indexes what it appends (hip_bamindex.h: BiWriterTap)
extern "C" int arx_bam_open_indexed(arx_ctx *ctx, const char *path, int32_t n_contigs, const char *const *names, const int32_t *lens, const char *extra_header, int32_t threads,
                                    int32_t level, int32_t flags, int32_t index, int32_t min_shift, const char *index_path, arx_bam **out, char *msg, int32_t msg_cap)
{
	auto say = [&](const std::string &m) { if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "%s", m.c_str()); };
	if (out) *out = nullptr;
	if (!ctx) { say("arx_bam_open_indexed: null context: the index is built on its GPU"); return ARX_E_ARG; }
	if (!out || !path || n_contigs < 0 || (n_contigs > 0 && (!names || !lens))) { say("arx_bam_open_indexed: null argument"); return ARX_E_ARG; }
	if (flags & ~(ARX_BAM_COORDINATE | ARX_BAM_DEVICE_SINK)) { say("arx_bam_open_indexed: unknown flag bits"); return ARX_E_ARG; }
	if (index != ARX_BAM_INDEX_BAI && index != ARX_BAM_INDEX_CSI && index != ARX_BAM_INDEX_AUTO) { say("arx_bam_open_indexed: index is ARX_BAM_INDEX_BAI, _CSI or _AUTO"); return ARX_E_ARG; }
	for (int32_t i = 0; i < n_contigs; ++i)
		if (lens[i] < 0) { say("arx_bam_open_indexed: contig " + std::to_string(i) + " has a negative length"); return ARX_E_ARG; }
	const int32_t too_long = arx::bi_long_contig(n_contigs, lens);
	const bool csi = index == ARX_BAM_INDEX_CSI || (index == ARX_BAM_INDEX_AUTO && too_long >= 0);
	if (!csi && too_long >= 0) { say(std::string(path) + ": " + arx::bi_long_text(too_long, lens[too_long])); return ARX_E_ARG; }
	const int32_t shift = csi ? arx::bi_csi_shift(min_shift) : 0;
	if (shift < 0) { say("arx_bam_open_indexed: min_shift lies outside [10, 24]"); return ARX_E_ARG; }
	const arx::BiScheme sc = csi ? arx::bi_csi_scheme(shift, n_contigs, lens) : arx::BI_BAI;
	const bool device_sink = (flags & ARX_BAM_DEVICE_SINK) != 0;
	arx::BamSink *w = nullptr;
	try {
		const int device = arx_ctx_device(ctx);
		std::unique_ptr<arx::BiWriterTap> tap(new arx::BiWriterTap());
		w = new arx::BamSink();
		w->coordinate = true;
		w->record_blocks = true;
		if (device_sink) w->comp = arx::shared_device_bgzf(device);
		if (!w->open(path, n_contigs, names, lens, extra_header, threads, device_sink ? 1 : level)) {
			const bool io = !device_sink || !w->f;
			say(w->error);
			delete w;
			return io ? ARX_E_IO : ARX_E_DEVICE;
		}
		tap->begin(device, sc, csi, index_path ? std::string(index_path) : std::string(path) + (csi ? ".csi" : ".bai"), n_contigs, lens, w->bytes_in); // (the header is all that went in)
		w->tap = std::move(tap);
	} catch (const std::exception &e) {
		say(e.what());
		delete w;
		return ARX_E_DEVICE;
	}
	*out = (arx_bam *)w;
	return ARX_OK;
}

extern "C" int arx_bam_sort_append(arx_ctx *ctx, arx_bam *h, const char *in_path, int32_t mode, int64_t max_bytes, int64_t *stats, char *msg, int32_t msg_cap)
{
	auto say = [&](const std::string &m) { if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "%s", m.c_str()); };
	if (stats) for (int k = 0; k < arx::BS_N_STATS; ++k) stats[k] = 0;
	arx::BamSink *w = (arx::BamSink *)h;
	const int32_t what = mode & ~ARX_SORT_TIMED;
	if (!ctx || !w || !in_path || max_bytes < 0 || (what != ARX_SORT_COORDINATE && what != ARX_SORT_COPY)) { say("arx_bam_sort_append: bad arguments"); return ARX_E_ARG; }
	std::string err;
	try {
		int32_t n = 0;
		const char *const *names = nullptr;
		const int64_t *offs = nullptr;
		const int32_t *lens = nullptr, *alt = nullptr;
		int64_t l_pac = 0;
		if (arx_contigs(ctx, &n, &names, &offs, &lens, &alt, &l_pac) != ARX_OK) { say("arx_bam_sort_append: the context has no contigs"); return ARX_E_ARG; }
		const bool device_writer = dynamic_cast<arx::DeviceBgzf *>(w->comp.get()) != nullptr;
		const int rc = arx::bs_sort_append(arx_ctx_device(ctx), w, device_writer, [&](const uint8_t *d, int64_t bytes, int64_t recs) { return bam_write_device(w, d, bytes, recs, true); },
		                                   in_path, mode, max_bytes, n, names, lens, stats, err);
		if (rc != ARX_OK) say(err);
		return rc;
	} catch (const arx::BsTooLarge &e) {
		say(e.what());
		return ARX_E_TOO_LARGE;
	} catch (const arx::HipOutOfMemory &e) { // any buffer of the sort (hip_res.h)
		say("the device memory does not hold the sort of this file (" + std::to_string(e.wanted >> 20) + " MiB more were asked for): use a smaller position bucket");
		return ARX_E_TOO_LARGE;
	} catch (const std::exception &e) {
		say(e.what());
		return ARX_E_DEVICE;
	}
}

extern "C" int arx_selftest_bam_sort(int32_t device, const uint8_t *stream, int64_t n_bytes, int32_t n_ref, int64_t seg_bytes, int32_t mode, uint8_t *out, int64_t *rec_off,
                                     int64_t *n_records, int64_t *stats)
{
	const int32_t what = mode & ~ARX_SORT_TIMED;
	if (n_bytes < 0 || n_ref < 0 || seg_bytes < arx::BS_MIN_SEG || (seg_bytes & (seg_bytes - 1)) || !n_records || !rec_off || (n_bytes > 0 && (!stream || !out)) ||
	    (what != ARX_SORT_COORDINATE && what != ARX_SORT_COPY))
		return ARX_E_ARG;
	*n_records = 0;
	if (stats) for (int k = 0; k < arx::BS_N_STATS; ++k) stats[k] = 0;
	try {
		arx::select_device(device, arx::BS_NO_DEVICE);
		arx::Stream st;
		st.create();
		arx::BsHipDrv drv; drv.st = st; drv.timed = (mode & ARX_SORT_TIMED) != 0;
		arx::DevBuf d_s((size_t)n_bytes);
		if (n_bytes) ARX_HIP_CHECK(hipMemcpyAsync(d_s.p, stream, (size_t)n_bytes, hipMemcpyHostToDevice, drv.st));
		const bool sort = what == ARX_SORT_COORDINATE;
		const double t0 = arx::bs_now_us();
		arx::BsSorted s;
		if (s.run(drv, d_s.as<uint8_t>(), n_bytes, 0, seg_bytes, n_ref, sort) != arx::BS_OK) return ARX_E_IO;
		ARX_HIP_CHECK(hipStreamSynchronize(drv.st));
		drv.us[arx::BS_T_TOTAL] = arx::bs_now_us() - t0;
		const int64_t N = s.found.n_records;
		if (n_bytes) ARX_HIP_CHECK(hipMemcpyAsync(out, sort ? s.out.p : d_s.p, (size_t)n_bytes, hipMemcpyDeviceToHost, drv.st));
		ARX_HIP_CHECK(hipMemcpyAsync(rec_off, sort ? (const void *)s.m.out_off : s.rec_off.p, (size_t)(N + 1) * 8, hipMemcpyDeviceToHost, drv.st));
		ARX_HIP_CHECK(hipStreamSynchronize(drv.st));
		*n_records = N;
		arx::bs_stats(stats, drv, N, n_bytes, 0, s.found.n_seg, s.found.right, s.found.repaired, s.found.rounds, 1);
	} catch (const arx::BsTooLarge &) {
		return ARX_E_TOO_LARGE;
	} catch (const arx::HipOutOfMemory &) {
		return ARX_E_TOO_LARGE;
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
	return ARX_OK;
}

// ---- the FASTQ file-pair calls (hip_fqsort.h, hip_fqstd.h, hip_fqprep.h): what their entries share at this edge
// a file entry's body under the family's refusals: what it throws becomes the code and the text in msg.  oom_what, oom_remedy: the call's own
// words around the figures of a device memory that does not suffice
template <class Body> static int fq_file_call(char *msg, int32_t msg_cap, const char *oom_what, const char *oom_remedy, Body body)
{
	auto say = [&](const std::string &m) { if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "%s", m.c_str()); };
	try {
		body();
		return ARX_OK;
	} catch (const arx::FsBadArg &e) {
		say(e.what());
		return ARX_E_ARG;
	} catch (const arx::FsTooLarge &e) {
		say(e.what());
		return ARX_E_TOO_LARGE;
	} catch (const arx::FsIoError &e) {
		say(e.what());
		return ARX_E_IO;
	} catch (const arx::HipOutOfMemory &e) { // any buffer of the call (hip_res.h)
		say(std::string(oom_what) + " (" + std::to_string(e.wanted >> 20) + " MiB more were asked for, " + std::to_string(e.free_bytes >> 20) + " MiB are free)" + oom_remedy);
		return ARX_E_TOO_LARGE;
	} catch (const std::exception &e) {
		say(e.what());
		return ARX_E_DEVICE;
	}
}
// a self-test's body: the codes alone
template <class Body> static int fq_selftest_call(Body body)
{
	try {
		return body();
	} catch (const arx::FsTooLarge &) {
		return ARX_E_TOO_LARGE;
	} catch (const arx::HipOutOfMemory &) {
		return ARX_E_TOO_LARGE;
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
}
[[noreturn]] static void fq_bad(const char *call, const std::string &what) { throw arx::FsBadArg(std::string(call) + ": " + what); }

static bool fs_same_file(const char *a, const char *b)
{
	if (!strcmp(a, b)) return true;
	struct stat sa, sb;
	return stat(a, &sa) == 0 && stat(b, &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
}
// the four paths of a call; need_out: the call writes (no CHECK, no DETECT), so the outputs are two files that are no inputs
static void fq_check_paths(const char *call, const char *const in[2], const char *const out[2], bool need_out, bool rest_ok = true)
{
	if (!in[0] || !in[1] || !rest_ok || (need_out && (!out[0] || !out[1]))) fq_bad(call, "null argument");
	if (!need_out) return;
	if (fs_same_file(out[0], out[1])) fq_bad(call, "the two output paths are the same file");
	for (int i = 0; i < 2; ++i)
		for (int o = 0; o < 2; ++o)
			if (fs_same_file(in[i], out[o])) fq_bad(call, std::string(out[o]) + " is an input and an output");
}
static void fq_check_run_bytes(const char *call, int64_t run_bytes)
{
	if (run_bytes < -1 || (run_bytes > 0 && run_bytes < arx::FS_MIN_WINDOW))
		fq_bad(call, "run_bytes is -1, 0 or at least the " + std::to_string(arx::FS_MIN_WINDOW) + " bytes of the smallest parse window");
}
static void fq_check_format(const char *call, int32_t format)
{
	if (format < ARX_FQSTD_AUTO || format > ARX_FQSTD_TELLSEQ) fq_bad(call, "format is ARX_FQSTD_AUTO, _HAPLOTAGGING, _STLFR or _TELLSEQ");
}
// a self-test's texts and record offsets to the caller's room of cap[f] bytes; a text that is longer is refused with `over`.  Everything is here:
// only now is anything of the caller's written
static int fq_hand_out(const std::vector<uint8_t> text[2], const std::vector<int64_t> off[2], int64_t bytes1, int64_t bytes2, int64_t N, int64_t cap1, int64_t cap2, int over,
                       uint8_t *out1, uint8_t *out2, int64_t *out_len, int64_t *rec_off1, int64_t *rec_off2, int64_t *n_records)
{
	if ((int64_t)text[0].size() != bytes1 || (int64_t)text[1].size() != bytes2 || (int64_t)off[0].size() != N + 1 || (int64_t)off[1].size() != N + 1) return ARX_E_DEVICE;
	if (bytes1 > cap1 || bytes2 > cap2) return over;
	if (bytes1) memcpy(out1, text[0].data(), (size_t)bytes1);
	if (bytes2) memcpy(out2, text[1].data(), (size_t)bytes2);
	memcpy(rec_off1, off[0].data(), (size_t)(N + 1) * 8); memcpy(rec_off2, off[1].data(), (size_t)(N + 1) * 8);
	out_len[0] = bytes1; out_len[1] = bytes2;
	*n_records = N;
	return ARX_OK;
}
// the output offsets of a sort's N records
static void fs_fetch_offsets(arx::FsHipDrv &drv, const arx::FsSortMem &m, int64_t N, std::vector<int64_t> off[2])
{
	for (int f = 0; f < 2; ++f) off[f].assign((size_t)N + 1, 0);
	if (N) { drv.fetch(off[0].data(), m.out1, (size_t)(N + 1) * 8); drv.fetch(off[1].data(), m.out2, (size_t)(N + 1) * 8); }
}

// ---- the sort of a FASTQ file pair by barcode (dev_fqsort.h, hip_fqsort.h)
extern "C" int arx_fastq_sort(int32_t device, const char *r1_in, const char *r2_in, const char *r1_out, const char *r2_out, int32_t flags, int64_t max_bytes, int64_t *stats,
                              char *msg, int32_t msg_cap)
{
	if (stats) for (int k = 0; k < arx::FS_N_STATS; ++k) stats[k] = 0;
	return fq_file_call(msg, msg_cap, "the device memory does not hold the sort of these files", arx::FS_REMEDY, [&]() {
		const char *call = "arx_fastq_sort", *in[2] = {r1_in, r2_in}, *out[2] = {r1_out, r2_out};
		if (flags & ~(ARX_FQSORT_BGZF | ARX_FQSORT_CHECK | ARX_FQSORT_GUNZIP_DEVICE | ARX_FQSORT_TIMED)) fq_bad(call, "unknown flag bits");
		fq_check_paths(call, in, out, !(flags & ARX_FQSORT_CHECK), max_bytes >= 0);
		arx::fs_sort_files(device, in, out, flags, max_bytes, stats, arx::shared_device_bgzf);
	});
}

extern "C" int arx_selftest_fastq_sort(int32_t device, const uint8_t *t1, int64_t n1, const uint8_t *t2, int64_t n2, int64_t window_bytes, int64_t slab_bytes, uint8_t *out1,
                                       uint8_t *out2, int64_t *out_len, int64_t *rec_off1, int64_t *rec_off2, int64_t *n_records, int64_t *stats)
{
	if (n1 < 0 || n2 < 0 || !out_len || !rec_off1 || !rec_off2 || !n_records || (n1 > 0 && (!t1 || !out1)) || (n2 > 0 && (!t2 || !out2)) || slab_bytes < 0 ||
	    (window_bytes != 0 && (window_bytes < arx::FS_MIN_WINDOW || window_bytes > arx::FS_MAX_WINDOW)))
		return ARX_E_ARG;
	if (stats) for (int k = 0; k < arx::FS_N_STATS; ++k) stats[k] = 0;
	return fq_selftest_call([&]() -> int {
		arx::select_device(device, arx::FS_NO_DEVICE);
		arx::Stream st;
		st.create();
		arx::FsHipDrv drv; drv.st = st;
		arx::DevBuf d1((size_t)n1), d2((size_t)n2);
		if (n1) ARX_HIP_CHECK(hipMemcpyAsync(d1.p, t1, (size_t)n1, hipMemcpyHostToDevice, drv.st));
		if (n2) ARX_HIP_CHECK(hipMemcpyAsync(d2.p, t2, (size_t)n2, hipMemcpyHostToDevice, drv.st));
		const arx::FsText T = {d1.as<uint8_t>(), d2.as<uint8_t>(), n1, n2};
		arx::FsMemSink sink;
		sink.init(drv.st);
		arx::FsCounts c{};
		arx::FsSortMem m{};
		arx::fs_run(drv, T, window_bytes ? window_bytes : arx::FS_WINDOW_DEFAULT, slab_bytes ? slab_bytes : arx::FS_SLAB_DEFAULT, &sink, c, m);
		std::vector<int64_t> off[2];
		fs_fetch_offsets(drv, m, c.n_records, off);
		const int rc = fq_hand_out(sink.text, off, c.bytes1, c.bytes2, c.n_records, n1, n2, ARX_E_DEVICE, out1, out2, out_len, rec_off1, rec_off2, n_records);
		if (rc == ARX_OK) arx::fs_stats(stats, drv, c, n1, n2, true);
		return rc;
	});
}

// ---- the same sort of a file pair that device memory does not hold: sorted runs in temporary files, merged on the device (dev_fqmerge.h)
extern "C" int arx_fastq_sort_ex(int32_t device, const char *r1_in, const char *r2_in, const char *r1_out, const char *r2_out, int32_t flags, int64_t max_bytes, int64_t run_bytes,
                                 const char *tmp_dir, int64_t *stats, char *msg, int32_t msg_cap)
{
	if (stats) for (int k = 0; k < arx::FX_N_STATS; ++k) stats[k] = 0;
	if (run_bytes == 0) return arx_fastq_sort(device, r1_in, r2_in, r1_out, r2_out, flags, max_bytes, stats, msg, msg_cap);
	return fq_file_call(msg, msg_cap, "the device memory does not hold a run of these files or the table of their records",
	                    ": use a smaller run_bytes; where the table of all records is what does not fit, sort per lane", [&]() {
		const char *call = "arx_fastq_sort_ex", *in[2] = {r1_in, r2_in}, *out[2] = {r1_out, r2_out};
		if (flags & ~(ARX_FQSORT_BGZF | ARX_FQSORT_CHECK | ARX_FQSORT_GUNZIP_DEVICE | ARX_FQSORT_TIMED)) fq_bad(call, "unknown flag bits");
		fq_check_paths(call, in, out, !(flags & ARX_FQSORT_CHECK), max_bytes >= 0);
		fq_check_run_bytes(call, run_bytes);
		arx::fx_sort_files(device, in, out, flags, max_bytes, run_bytes, tmp_dir, stats, arx::shared_device_bgzf);
	});
}

extern "C" int arx_selftest_fastq_sort_ext(int32_t device, const uint8_t *t1, int64_t n1, const uint8_t *t2, int64_t n2, int64_t window_bytes, int64_t slab_bytes, int64_t run_bytes,
                                           uint8_t *out1, uint8_t *out2, int64_t *out_len, int64_t *rec_off1, int64_t *rec_off2, int64_t *n_records, int64_t *stats)
{
	const int64_t window = window_bytes ? window_bytes : run_bytes < arx::FS_WINDOW_DEFAULT ? run_bytes : arx::FS_WINDOW_DEFAULT; // 0: arx_fastq_sort_ex's
	if (n1 < 0 || n2 < 0 || !out_len || !rec_off1 || !rec_off2 || !n_records || (n1 > 0 && (!t1 || !out1)) || (n2 > 0 && (!t2 || !out2)) || slab_bytes < 0 ||
	    window < arx::FS_MIN_WINDOW || window > arx::FS_MAX_WINDOW || run_bytes < window)
		return ARX_E_ARG;
	if (stats) for (int k = 0; k < arx::FX_N_STATS; ++k) stats[k] = 0;
	return fq_selftest_call([&]() -> int {
		arx::select_device(device, arx::FS_NO_DEVICE);
		arx::Stream st;
		st.create();
		arx::FxHipDrv drv; drv.st = st;
		arx::FxMemSrc src(st, t1, n1, t2, n2);
		arx::FxMemStore store;
		arx::FsMemSink sink;
		sink.init(drv.st);
		arx::FxIo io;
		arx::FsCounts c{};
		arx::FsSortMem m{};
		arx::FxRuns S;
		arx::fx_run(drv, src, &store, &sink, run_bytes, window, slab_bytes ? slab_bytes : arx::FS_SLAB_DEFAULT, c, m, S, io);
		std::vector<int64_t> off[2];
		fs_fetch_offsets(drv, m, c.n_records, off);
		const int rc = fq_hand_out(sink.text, off, c.bytes1, c.bytes2, c.n_records, n1, n2, ARX_E_DEVICE, out1, out2, out_len, rec_off1, rec_off2, n_records);
		if (rc == ARX_OK) arx::fx_stats(stats, drv, c, n1, n2, true, S, io);
		return rc;
	});
}

// ---- in front of the sort: haplotagging, stLFR and TELLseq headers rewritten to the feeder's form (dev_fqstd.h, hip_fqstd.h)
extern "C" int arx_fastq_standardize(int32_t device, const char *r1_in, const char *r2_in, const char *r1_out, const char *r2_out, int32_t format, int32_t flags, int64_t *stats,
                                     char *msg, int32_t msg_cap)
{
	if (stats) for (int k = 0; k < arx::FQS_N_STATS; ++k) stats[k] = 0;
	return fq_file_call(msg, msg_cap, "the device memory does not hold the windows and slabs of the call", "", [&]() {
		const char *call = "arx_fastq_standardize", *in[2] = {r1_in, r2_in}, *out[2] = {r1_out, r2_out};
		if (flags & ~(ARX_FQSTD_BGZF | ARX_FQSTD_DETECT | ARX_FQSTD_GUNZIP_DEVICE | ARX_FQSTD_TIMED)) fq_bad(call, "unknown flag bits");
		fq_check_format(call, format);
		fq_check_paths(call, in, out, !(flags & ARX_FQSTD_DETECT));
		arx::fqs_files(device, in, out, format, flags, stats, arx::shared_device_bgzf);
	});
}

extern "C" int arx_selftest_fastq_standardize(int32_t device, const uint8_t *t1, int64_t n1, const uint8_t *t2, int64_t n2, int32_t format, int64_t window_bytes, int64_t slab_bytes,
                                              uint8_t *out1, int64_t cap1, uint8_t *out2, int64_t cap2, int64_t *out_len, int64_t *rec_off1, int64_t *rec_off2, int64_t *n_records,
                                              int64_t *stats)
{
	if (n1 < 0 || n2 < 0 || cap1 < 0 || cap2 < 0 || !out_len || !rec_off1 || !rec_off2 || !n_records || (n1 > 0 && !t1) || (n2 > 0 && !t2) || (cap1 > 0 && !out1) || (cap2 > 0 && !out2) ||
	    slab_bytes < 0 || format < ARX_FQSTD_AUTO || format > ARX_FQSTD_TELLSEQ || (window_bytes != 0 && (window_bytes < arx::FS_MIN_WINDOW || window_bytes > arx::FS_MAX_WINDOW)))
		return ARX_E_ARG;
	if (stats) for (int k = 0; k < arx::FQS_N_STATS; ++k) stats[k] = 0;
	const int64_t window = window_bytes ? window_bytes : arx::FS_WINDOW_DEFAULT, slab = slab_bytes ? slab_bytes : arx::FS_SLAB_DEFAULT;
	return fq_selftest_call([&]() -> int {
		arx::select_device(device, arx::FQS_NO_DEVICE);
		arx::Stream st;
		st.create();
		arx::FqsHipDrv drv; drv.st = st;
		int fmt = format;
		int64_t decided = -1;
		if (format == ARX_FQSTD_AUTO) {
			arx::FqsCounts d;
			arx::fqs_detect_mem(drv, t1, n1, t2, n2, window, d);
			fmt = d.format; decided = d.decided;
			if (fmt == ARX_FQSTD_STANDARD || fmt == ARX_FQSTD_UNKNOWN) {
				d.n_records = 0; // nothing was written
				arx::fqs_stats(stats, drv, d, fmt, decided, 0, 0, 0);
				return fmt == ARX_FQSTD_STANDARD ? ARX_OK : ARX_E_ARG;
			}
		}
		arx::FxMemSrc src(st, t1, n1, t2, n2);
		arx::FsMemSink sink;
		sink.init(drv.st);
		arx::FqsCounts c;
		std::vector<int64_t> off[2];
		c.off1 = &off[0]; c.off2 = &off[1];
		arx::fqs_throw(arx::fqs_convert(drv, src, fmt, window, slab, sink, c), window);
		sink.flush();
		drv.pass_done();
		const int rc = fq_hand_out(sink.text, off, c.bytes1, c.bytes2, c.n_records, cap1, cap2, ARX_E_TOO_LARGE, out1, out2, out_len, rec_off1, rec_off2, n_records);
		if (rc == ARX_OK) arx::fqs_stats(stats, drv, c, fmt, decided, sink.us_consume, 0, 0);
		return rc;
	});
}

// ---- the step that opens every run: the reference FASTA read and packed on the device (dev_fapack.h, hip_fapack.h; replaces bntseq.c:227-328)
extern "C" int arx_index_build_ex(int32_t device, const char *fasta, const char *prefix, int32_t flags, int64_t *stats, char *msg, int32_t msg_cap)
{
	if (stats) for (int k = 0; k < arx::FA_N_STATS; ++k) stats[k] = 0;
	std::string refused; // what arx_index_build refuses too: its code and its texts
	const int rc = fq_file_call(msg, msg_cap, "the device memory does not hold the packed strand and the windows of the call", "", [&]() {
		const char *call = "arx_index_build_ex";
		if (!fasta || !prefix) fq_bad(call, "null argument");
		if (flags & ~ARX_INDEX_PACK_ONLY) fq_bad(call, "unknown flag bits");
		try {
			arx::fa_build_files(device, fasta, prefix, flags, stats);
		} catch (const arx::FaRefused &e) {
			refused = e.what();
		}
	});
	if (refused.empty()) return rc;
	if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "%s", refused.c_str());
	return ARX_E_OPEN;
}

extern "C" int arx_selftest_fasta_pack(int32_t device, const uint8_t *text, int64_t n, int64_t window_bytes, uint8_t *pac, int64_t pac_cap, int64_t *out, int64_t *contig_rows,
                                       int64_t contig_cap, int64_t *hole_rows, int64_t hole_cap)
{
	if (n < 0 || (n > 0 && !text) || !out || pac_cap < 0 || contig_cap < 0 || hole_cap < 0 || (pac_cap > 0 && !pac) || (contig_cap > 0 && !contig_rows) || (hole_cap > 0 && !hole_rows) ||
	    (window_bytes != 0 && (window_bytes < arx::FA_MIN_WINDOW || window_bytes > arx::FA_MAX_WINDOW)))
		return ARX_E_ARG;
	for (int k = 0; k < 10; ++k) out[k] = 0;
	return fq_selftest_call([&]() -> int {
		arx::select_device(device, arx::FA_NO_DEVICE);
		arx::Stream st;
		st.create();
		arx::FaHipDrv drv; drv.st = st;
		arx::FaState S;
		std::vector<arx::FaContig> contigs;
		std::vector<arx::FaHole> holes;
		std::vector<uint8_t> bytes;
		arx::fa_pack_mem(drv, text, n, window_bytes ? window_bytes : arx::FA_WINDOW_DEFAULT, S, contigs, holes, bytes);
		out[8] = S.windows;
		if (S.bad_start || S.l_pac == 0) { out[9] = S.bad_start ? 1 : 2; return ARX_E_OPEN; }
		if (S.contig_too_long || (int64_t)bytes.size() > pac_cap || (int64_t)contigs.size() > contig_cap || (int64_t)holes.size() > hole_cap) return ARX_E_TOO_LARGE;
		if (!bytes.empty()) memcpy(pac, bytes.data(), bytes.size());
		out[0] = S.l_pac; out[1] = S.n_contigs; out[2] = S.n_holes; out[3] = S.n_amb;
		for (int c = 0; c < 4; ++c) out[4 + c] = (int64_t)S.cnt[c];
		for (size_t c = 0; c < contigs.size(); ++c) {
			const arx::FaContig &r = contigs[c];
			const int64_t row[5] = {r.hdr_b, r.hdr_e, r.off, r.len, r.n_holes};
			memcpy(contig_rows + 5 * c, row, sizeof row);
		}
		for (size_t h = 0; h < holes.size(); ++h) { hole_rows[3 * h] = holes[h].off; hole_rows[3 * h + 1] = holes[h].len; hole_rows[3 * h + 2] = holes[h].ch; }
		return ARX_OK;
	});
}

// ---- the two in one call: raw headers in, standardized records ordered by barcode out (dev_fqprep.h, hip_fqprep.h)
extern "C" int arx_fastq_prepare(int32_t device, const char *r1_in, const char *r2_in, const char *r1_out, const char *r2_out, int32_t format, int32_t flags, int64_t max_bytes,
                                 int64_t run_bytes, const char *tmp_dir, int64_t *stats, char *msg, int32_t msg_cap)
{
	if (stats) for (int k = 0; k < arx::FP_N_STATS; ++k) stats[k] = 0;
	return fq_file_call(msg, msg_cap, "the device memory does not hold these files, a run of them or the table of their records",
	                    ": prepare in runs (run_bytes -1), or with a smaller run_bytes; where the table of all records is what does not fit, prepare per lane", [&]() {
		const char *call = "arx_fastq_prepare", *in[2] = {r1_in, r2_in}, *out[2] = {r1_out, r2_out};
		if (flags & ~(ARX_FQSORT_BGZF | ARX_FQSORT_CHECK | ARX_FQSORT_GUNZIP_DEVICE | ARX_FQSORT_TIMED)) fq_bad(call, "unknown flag bits");
		fq_check_format(call, format);
		fq_check_paths(call, in, out, !(flags & ARX_FQSORT_CHECK), max_bytes >= 0);
		fq_check_run_bytes(call, run_bytes);
		arx::fp_files(device, in, out, format, flags, max_bytes, run_bytes, tmp_dir, stats, arx::shared_device_bgzf);
	});
}

extern "C" int arx_selftest_fastq_prepare(int32_t device, const uint8_t *t1, int64_t n1, const uint8_t *t2, int64_t n2, int32_t format, int64_t window_bytes, int64_t slab_bytes,
                                          int64_t run_bytes, uint8_t *out1, int64_t cap1, uint8_t *out2, int64_t cap2, int64_t *out_len, int64_t *rec_off1, int64_t *rec_off2,
                                          int64_t *n_records, int64_t *stats)
{
	const int64_t window = window_bytes ? window_bytes : run_bytes > 0 && run_bytes < arx::FS_WINDOW_DEFAULT ? run_bytes : arx::FS_WINDOW_DEFAULT; // 0: arx_fastq_prepare's
	const int64_t slab = slab_bytes ? slab_bytes : arx::FS_SLAB_DEFAULT;
	if (n1 < 0 || n2 < 0 || cap1 < 0 || cap2 < 0 || !out_len || !rec_off1 || !rec_off2 || !n_records || (n1 > 0 && !t1) || (n2 > 0 && !t2) || (cap1 > 0 && !out1) || (cap2 > 0 && !out2) ||
	    slab_bytes < 0 || format < ARX_FQSTD_AUTO || format > ARX_FQSTD_TELLSEQ || window < arx::FS_MIN_WINDOW || window > arx::FS_MAX_WINDOW || run_bytes < 0 ||
	    (run_bytes != 0 && run_bytes < window))
		return ARX_E_ARG;
	if (stats) for (int k = 0; k < arx::FP_N_STATS; ++k) stats[k] = 0;
	return fq_selftest_call([&]() -> int {
		arx::select_device(device, arx::FP_NO_DEVICE);
		arx::Stream st;
		st.create();
		arx::FpHipDrv drv; drv.st = st;
		int fmt = format;
		int64_t decided = -1;
		arx::FpRows rows;
		std::vector<int64_t> off[2];
		if (format == ARX_FQSTD_AUTO) {
			arx::FqsCounts d;
			arx::fqs_detect_mem(drv, t1, n1, t2, n2, window, d);
			fmt = d.format; decided = d.decided;
			if (fmt == ARX_FQSTD_UNKNOWN) {
				arx::fp_stats(stats, fmt, -1, rows);
				return ARX_E_ARG;
			}
			if (fmt == ARX_FQSTD_STANDARD) { // the sort itself, into room of its own: the caller's is written only when everything is here
				std::vector<uint8_t> o[2] = {std::vector<uint8_t>((size_t)n1 + 1), std::vector<uint8_t>((size_t)n2 + 1)};
				for (int f = 0; f < 2; ++f) off[f].resize((size_t)(n1 / 5 + 2));
				int64_t len[2] = {0, 0}, N = 0, s[arx::FX_N_STATS] = {0};
				int rc = run_bytes == 0 ? arx_selftest_fastq_sort(device, t1, n1, t2, n2, window, slab, o[0].data(), o[1].data(), len, off[0].data(), off[1].data(), &N, s)
				                        : arx_selftest_fastq_sort_ext(device, t1, n1, t2, n2, window, slab, run_bytes, o[0].data(), o[1].data(), len, off[0].data(), off[1].data(), &N, s);
				if (rc != ARX_OK) return rc;
				for (int f = 0; f < 2; ++f) { o[f].resize((size_t)len[f]); off[f].resize((size_t)N + 1); }
				rc = fq_hand_out(o, off, len[0], len[1], N, cap1, cap2, ARX_E_TOO_LARGE, out1, out2, out_len, rec_off1, rec_off2, n_records);
				if (rc != ARX_OK) return rc;
				if (stats) memcpy(stats, s, sizeof s);
				arx::fp_stats(stats, fmt, decided, rows);
				return ARX_OK;
			}
		}
		rows.format = fmt;
		arx::FsMemSink sink;
		sink.init(drv.st);
		arx::FsCounts c{};
		arx::FsSortMem m{};
		arx::FxRuns S;
		arx::FxIo io;
		arx::FxMemStore store;
		arx::DevBuf d1, d2;
		if (run_bytes == 0) {
			d1.alloc((size_t)n1); d2.alloc((size_t)n2);
			if (n1) ARX_HIP_CHECK(hipMemcpyAsync(d1.p, t1, (size_t)n1, hipMemcpyHostToDevice, drv.st));
			if (n2) ARX_HIP_CHECK(hipMemcpyAsync(d2.p, t2, (size_t)n2, hipMemcpyHostToDevice, drv.st));
			const arx::FsText T = {d1.as<uint8_t>(), d2.as<uint8_t>(), n1, n2};
			arx::fs_run_by(drv, T, window, slab, &sink, c, m, rows);
		} else {
			arx::FxMemSrc src(st, t1, n1, t2, n2);
			arx::fx_run_by(drv, src, &store, &sink, run_bytes, window, slab, c, m, S, io, rows);
		}
		fs_fetch_offsets(drv, m, c.n_records, off);
		const int rc = fq_hand_out(sink.text, off, c.bytes1, c.bytes2, c.n_records, cap1, cap2, ARX_E_TOO_LARGE, out1, out2, out_len, rec_off1, rec_off2, n_records);
		if (rc != ARX_OK) return rc;
		arx::fx_stats(stats, drv, c, n1, n2, true, S, io);
		arx::fp_stats(stats, fmt, decided, rows);
		return ARX_OK;
	});
}

// ---- the .bai or the .csi of a coordinate-sorted BAM file (dev_bamindex.h, hip_bamindex.h).  csi_shift: 0 for the .bai, else the .csi's min_shift
static int bam_index_file(const char *entry, int32_t device, const char *bam_path, const char *index_path, int32_t csi_shift, int64_t max_bytes, int32_t flags, int64_t *stats, char *msg,
                          int32_t msg_cap)
{
	auto say = [&](const std::string &m) { if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "%s", m.c_str()); };
	if (stats) for (int k = 0; k < arx::BI_N_STATS; ++k) stats[k] = 0;
	if (flags & ~ARX_BAI_TIMED) { say(std::string(entry) + ": unknown flag bits"); return ARX_E_ARG; }
	if (!bam_path || max_bytes < 0) { say(std::string(entry) + ": bad arguments"); return ARX_E_ARG; }
	if (csi_shift < 0) { say(std::string(entry) + ": min_shift lies outside [10, 24]"); return ARX_E_ARG; }
	std::string err;
	try {
		const int rc = arx::bi_index_file(device, bam_path, index_path, max_bytes, (flags & ARX_BAI_TIMED) != 0, stats, err, csi_shift);
		if (rc != ARX_OK) say(err);
		return rc;
	} catch (const arx::BsTooLarge &e) {
		say(e.what());
		return ARX_E_TOO_LARGE;
	} catch (const arx::HipOutOfMemory &e) { // any buffer of a slab (hip_res.h)
		say("the device memory does not hold a slab of this file (" + std::to_string(e.wanted >> 20) + " MiB more were asked for): use a smaller max_bytes");
		return ARX_E_TOO_LARGE;
	} catch (const std::exception &e) {
		say(e.what());
		return ARX_E_DEVICE;
	}
}
extern "C" int arx_bam_index(int32_t device, const char *bam_path, const char *bai_path, int64_t max_bytes, int32_t flags, int64_t *stats, char *msg, int32_t msg_cap)
{
	return bam_index_file("arx_bam_index", device, bam_path, bai_path, 0, max_bytes, flags, stats, msg, msg_cap);
}
extern "C" int arx_bam_index_csi(int32_t device, const char *bam_path, const char *csi_path, int32_t min_shift, int64_t max_bytes, int32_t flags, int64_t *stats, char *msg, int32_t msg_cap)
{
	return bam_index_file("arx_bam_index_csi", device, bam_path, csi_path, arx::bi_csi_shift(min_shift), max_bytes, flags, stats, msg, msg_cap);
}

static int selftest_bam_index(int32_t device, const uint8_t *stream, int64_t n_bytes, int64_t hdr, int32_t n_ref, const int32_t *ref_len, int64_t n_blocks, const int64_t *blk_at,
                              const int32_t *blk_isize, int64_t seg_bytes, int64_t slab_bytes, int32_t csi_shift, uint8_t *out, int64_t out_cap, int64_t *out_len, int64_t *stats)
{
	if (csi_shift < 0 || n_bytes < 0 || hdr < 0 || hdr > n_bytes || n_ref < 0 || (n_ref > 0 && !ref_len) || n_blocks < 0 || !blk_at || (n_blocks > 0 && !blk_isize) || seg_bytes < arx::BS_MIN_SEG ||
	    (seg_bytes & (seg_bytes - 1)) || slab_bytes < 0 || out_cap < 0 || (out_cap > 0 && !out) || !out_len || (n_bytes > 0 && !stream))
		return ARX_E_ARG;
	*out_len = 0;
	if (stats) for (int k = 0; k < arx::BI_N_STATS; ++k) stats[k] = 0;
	int64_t sum = 0;
	for (int64_t b = 0; b < n_blocks; ++b) {
		if (blk_isize[b] < 0 || blk_isize[b] > arx::INF_MAX_OUT || blk_at[b] > blk_at[b + 1]) return ARX_E_ARG;
		sum += blk_isize[b];
	}
	const bool csi = csi_shift != 0;
	if (sum != n_bytes || (!csi && arx::bi_long_contig(n_ref, ref_len) >= 0)) return ARX_E_ARG;
	for (int32_t i = 0; i < n_ref; ++i)
		if (ref_len[i] < 0) return ARX_E_ARG;
	const arx::BiScheme sc = csi ? arx::bi_csi_scheme(csi_shift, n_ref, ref_len) : arx::BI_BAI;
	arx::BiBlocks B;
	if (!B.build(n_blocks, blk_at, blk_isize, slab_bytes)) return ARX_E_ARG;
	try {
		arx::select_device(device, arx::BI_NO_DEVICE);
		arx::Stream st;
		st.create();
		arx::BiHipDrv drv; drv.st = st;
		const double t0 = arx::bs_now_us();
		arx::DevBuf d_s((size_t)n_bytes);
		drv.upload(d_s.p, stream, (size_t)n_bytes);
		arx::BiIndex ix;
		arx::BiMemSrc src{drv, d_s.as<uint8_t>(), B};
		std::string err;
		const int rc = arx::bi_result(arx::bi_run(drv, src, B, hdr, n_ref, ref_len, seg_bytes, ix, sc), ix, "the stream", err);
		if (rc != ARX_OK) {
			if (stats) stats[9] = (int64_t)ix.err; // the first offending record's number << 8 | the rule, or -1
			return rc;
		}
		const std::vector<uint8_t> bai = csi ? arx::bi_serialise_csi(ix) : arx::bi_serialise(ix);
		if ((int64_t)bai.size() > out_cap) return ARX_E_TOO_LARGE;
		memcpy(out, bai.data(), bai.size());
		*out_len = (int64_t)bai.size();
		drv.us[arx::BI_T_TOTAL] = arx::bs_now_us() - t0;
		arx::bi_stats(stats, drv, ix, n_bytes, n_blocks);
		if (csi) arx::bi_stats_csi(stats, sc);
	} catch (const arx::BsTooLarge &) {
		return ARX_E_TOO_LARGE;
	} catch (const arx::HipOutOfMemory &) {
		return ARX_E_TOO_LARGE;
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
	return ARX_OK;
}
extern "C" int arx_selftest_bam_index(int32_t device, const uint8_t *stream, int64_t n_bytes, int64_t hdr, int32_t n_ref, const int32_t *ref_len, int64_t n_blocks,
                                      const int64_t *blk_at, const int32_t *blk_isize, int64_t seg_bytes, int64_t slab_bytes, uint8_t *out, int64_t out_cap, int64_t *out_len,
                                      int64_t *stats)
{
	return selftest_bam_index(device, stream, n_bytes, hdr, n_ref, ref_len, n_blocks, blk_at, blk_isize, seg_bytes, slab_bytes, 0, out, out_cap, out_len, stats);
}
extern "C" int arx_selftest_bam_index_csi(int32_t device, const uint8_t *stream, int64_t n_bytes, int64_t hdr, int32_t n_ref, const int32_t *ref_len, int64_t n_blocks,
                                          const int64_t *blk_at, const int32_t *blk_isize, int64_t seg_bytes, int64_t slab_bytes, int32_t min_shift, uint8_t *out, int64_t out_cap,
                                          int64_t *out_len, int64_t *stats)
{
	return selftest_bam_index(device, stream, n_bytes, hdr, n_ref, ref_len, n_blocks, blk_at, blk_isize, seg_bytes, slab_bytes, arx::bi_csi_shift(min_shift), out, out_cap, out_len, stats);
}

// the index a writer builds of what it is handed (dev_bamindex.h: BiPush), on a stream in host memory and a table of the writer's layout
extern "C" int arx_selftest_bam_index_feeds(int32_t device, const uint8_t *stream, int64_t n_bytes, int64_t hdr, int32_t n_ref, const int32_t *ref_len, int64_t n_blocks,
                                            const int64_t *blk_at, int64_t seg_bytes, int64_t n_feeds, const int64_t *feed_end, int64_t piece_bytes, int32_t min_shift, uint8_t *out,
                                            int64_t out_cap, int64_t *out_len, int64_t *stats)
{
	const bool csi = min_shift != -1;
	const int32_t csi_shift = csi ? arx::bi_csi_shift(min_shift) : 0;
	if (csi_shift < 0 || n_bytes < 0 || hdr < 0 || hdr > n_bytes || n_ref < 0 || (n_ref > 0 && !ref_len) || n_blocks < 0 || !blk_at || seg_bytes < arx::BS_MIN_SEG ||
	    (seg_bytes & (seg_bytes - 1)) || n_feeds < 1 || !feed_end || piece_bytes < 0 || out_cap < 0 || (out_cap > 0 && !out) || !out_len || (n_bytes > 0 && !stream))
		return ARX_E_ARG;
	*out_len = 0;
	if (stats) for (int k = 0; k < arx::BI_N_STATS; ++k) stats[k] = 0;
	if (n_blocks != arx::bi_header_blocks(hdr) + (n_bytes - hdr + arx::BI_BLOCK - 1) / arx::BI_BLOCK) return ARX_E_ARG; // the writer's layout
	for (int64_t b = 0; b <= n_blocks; ++b)
		if (blk_at[b] < 0 || blk_at[b] >= arx::BI_MAX_AT || (b > 0 && blk_at[b] <= blk_at[b - 1])) return ARX_E_ARG;
	for (int64_t k = 0; k < n_feeds; ++k)
		if (feed_end[k] < 0 || feed_end[k] > n_bytes || (k > 0 && feed_end[k] < feed_end[k - 1])) return ARX_E_ARG;
	if (feed_end[n_feeds - 1] != n_bytes || (!csi && arx::bi_long_contig(n_ref, ref_len) >= 0)) return ARX_E_ARG;
	for (int32_t i = 0; i < n_ref; ++i)
		if (ref_len[i] < 0) return ARX_E_ARG;
	const arx::BiScheme sc = csi ? arx::bi_csi_scheme(csi_shift, n_ref, ref_len) : arx::BI_BAI;
	try {
		arx::select_device(device, arx::BI_NO_DEVICE);
		arx::Stream st;
		st.create();
		arx::BiHipDrv drv; drv.st = st;
		const double t0 = arx::bs_now_us();
		arx::DevBuf d_s((size_t)n_bytes);
		drv.upload(d_s.p, stream, (size_t)n_bytes);
		arx::BiPush<arx::BiHipDrv> push;
		push.begin(drv, n_ref, ref_len, sc, hdr, seg_bytes, piece_bytes);
		int bi = arx::BI_OK;
		int64_t at = hdr;
		for (int64_t k = 0; k < n_feeds && bi == arx::BI_OK; ++k) {
			if (feed_end[k] <= at) continue; // an end inside the header, or an empty feed
			bi = push.feed(drv, d_s.as<uint8_t>() + at, feed_end[k] - at);
			at = feed_end[k];
		}
		if (bi == arx::BI_OK) bi = push.finish(drv, blk_at);
		std::string err;
		const int rc = arx::bi_result(bi, push.ix, "the stream", err);
		if (rc != ARX_OK) {
			if (stats) stats[9] = (int64_t)push.ix.err; // the first offending record's number << 8 | the rule, or -1
			return rc;
		}
		const std::vector<uint8_t> bytes = csi ? arx::bi_serialise_csi(push.ix) : arx::bi_serialise(push.ix);
		if ((int64_t)bytes.size() > out_cap) return ARX_E_TOO_LARGE;
		memcpy(out, bytes.data(), bytes.size());
		*out_len = (int64_t)bytes.size();
		drv.us[arx::BI_T_TOTAL] = arx::bs_now_us() - t0;
		arx::bi_stats(stats, drv, push.ix, n_bytes, n_blocks);
		if (csi) arx::bi_stats_csi(stats, sc);
	} catch (const arx::BsTooLarge &) {
		return ARX_E_TOO_LARGE;
	} catch (const arx::HipOutOfMemory &) {
		return ARX_E_TOO_LARGE;
	} catch (const std::exception &) {
		return ARX_E_DEVICE;
	}
	return ARX_OK;
}

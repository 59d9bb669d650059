// device_feeder.h -- the FASTQ feeder whose per-byte work runs on the device (arx_feeder_open_device): what feeder.h's Feeder does on
// one host thread per file pair, re-shaped so that ONE file pair can feed several workers.
//
//   two reader threads (feeder.h)        ChunkReader: inflate R1 and R2 side by side into page-locked buffers, chunk by chunk; or, for a
//                                         BGZF file of a feeder opened with ARX_FEEDER_INFLATE_DEVICE, BgzfChunkReader: whole blocks as
//                                         they are in the file, with one table row per block
//                                         or, for an ordinary gzip file of a feeder opened with ARX_FEEDER_GUNZIP_DEVICE, GzipRawReader: the
//                                         next bytes of the file as they are, which a GzReader (gunzip_host.h) takes a launch at a time
//   step()                                uploads what both readers have; a BGZF slab's blocks are inflated on the device (dev_inflate.h),
//                                         straight into the window behind the carry, so that the parse sees text either way
//   parse_window()                        uploads what both readers have, runs dev_fastq.h's functors on the raw text (line index, record
//                                         recognition, header fields, base codes, barcode runs) and copies one output blob home
//   next()                                ReadBarcodeSet's rules (feeder.h:141-169) applied to the run list on the host; whole sets are
//                                         handed out from one of depth + 2 slots, the reads of a super-batch contiguous in device memory
//
// Chunks of the two files cover different line ranges: a parse consumes the lines both windows hold, up to the last record that is
// complete in both, and carries the rest of either window forward in device memory (a record that the windows cut off is carried whole,
// so every parse starts in the search state).  What the host waits for per parse, whatever the number of chunks it takes in: the upload,
// the two line counts, the record count, the output sizes and the output blob (each of the three scans is two waits inside the runtime).
//
// Ordinary gzip on the device (ARX_FEEDER_GUNZIP_DEVICE).  Each such file has a GzReader over its raw slabs and a backend with a stream of its
// own; a piece of text is what one launch accepts, resolved straight into the window behind the carry, and a file is asked for pieces while
// its window holds less than chunk_bytes.  step() enqueues find / decode / windows of every file that wants a piece before it waits for any
// (GzReader::begin), makes room for the texts, enqueues the resolves (place_begin), waits, and parses.  Whatever the device does not take
// is the host's inside GzReader (zlib), as in the file calls; where the reader reports an error the input ends there like at a read error.
// A piece that has entered a parse cannot be taken back: can_rewind stays false, a member whose trailer does not match is an error.
//   The compressed bytes per launch (the slab): a launch runs one wavefront per 32 KiB chunk, so the slab is as large as chunk_bytes lets it
// be -- chunk_bytes itself, at least two chunks, at most GZ_SLAB_DEFAULT (8 MiB) and gunzip_host.h's other bounds.  At FASTQ's usual ratio a
// piece is then three to four times chunk_bytes of text, which the window takes (its 2^30 check applies as before).  No value of the slab or
// of the chunk has been measured through the feeder.  ARX_FEEDER_GUNZIP_CHUNK / ARX_FEEDER_GUNZIP_SLAB set the two (tests: many chunks and
// launches in a small file); values outside arx_selftest_gunzip's bounds are refused at open.
//
// Compiled for the GPU into arx_api.hip and, with the sequential runtime, into the host test double: the same code either way.
#pragma once
#include <chrono>
#include <deque>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "feeder.h"
#include "dev_fastq.h"
#include "switches.h"
#include "gunzip_host.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
#include "dev_inflate.h"
#endif

namespace arx {

// The inflate of a slab's BGZF blocks, enqueued on the runtime's stream: the HIP kernel (hip_inflate.h, compiled in arx_bgzf.hip) with the HIP
// runtime, the same dev_inflate.h functions with the lanes in a loop with the sequential runtime of the host test double.  Everything is
// device memory; counts[0] is raised per block that is not INF_OK, counts[1] by the DEFLATE blocks read
#if defined(__HIPCC__)
void inflate_launch(hipStream_t stream, const uint8_t *d_src, int64_t src_bytes, const InfRow *d_rows, int n_blocks, uint8_t *d_out, int64_t out_bytes, int32_t *d_status,
                    int32_t *d_counts);
template <class RT> inline void inflate_rows(RT &rt, const uint8_t *src, int64_t src_bytes, const InfRow *rows, int n, uint8_t *out, int64_t out_bytes, int32_t *status, int32_t *counts)
{
	typename RT::Scope sc(rt, "bgzf_inflate", n);
	inflate_launch(rt.stream, src, src_bytes, rows, n, out, out_bytes, status, counts);
}
#else
struct InfLoopDrv { template <class F> void lanes(F f) { for (int l = 0; l < INF_LANES; ++l) f(l); } };
template <class RT> inline void inflate_rows(RT &, const uint8_t *src, int64_t src_bytes, const InfRow *rows, int n, uint8_t *out, int64_t out_bytes, int32_t *status, int32_t *counts)
{
	std::vector<uint8_t> mem(INF_WORK_BYTES + 4), lds_out(INF_MAX_OUT);
	InfWork w;
	inf_carve(w, mem.data() + ((4 - ((uintptr_t)mem.data() & 3)) & 3), lds_out.data());
	InfLoopDrv drv;
	for (int b = 0; b < n; ++b) {
		const InfRow &r = rows[b];
		int st = INF_BAD_HEADER, nd = 0;
		if (inf_row_in_range(r, src_bytes, out_bytes)) st = inf_block(drv, w, src + r.coff, r.clen, r.isize, r.crc, out + r.ooff, &nd);
		status[b] = st;
		if (st != INF_OK) ++counts[0];
		counts[1] += nd;
	}
}
#endif

// The backend of a gzip file's GzReader, in the halves gunzip_host.h describes.  With the HIP runtime: hip_gunzip.h's GzHip on a stream of its
// own, behind functions that arx_bgzf.hip defines next to the kernels (as inflate_launch); `after` is the feeder's stream, on which the
// window is made and parsed.  With the sequential runtime of the host test double: dev_gunzip.h's functions with lanes and chunks in a loop.
#if defined(__HIPCC__)
struct GzFeedDev;
GzFeedDev *gz_feed_open();
void gz_feed_close(GzFeedDev *d);
void gz_feed_decode_begin(GzFeedDev *d, const uint8_t *src, int clen, int start_bit, const uint8_t *window, int have, int chunk_bytes, int expand);
void gz_feed_decode_end(GzFeedDev *d, GzLaunch &L);
void gz_feed_resolve_begin(GzFeedDev *d, GzLaunch &L, uint8_t *text, hipStream_t after);
void gz_feed_resolve_end(GzFeedDev *d, GzLaunch &L);
void gz_feed_upload(GzFeedDev *d, uint8_t *dst, const uint8_t *host, size_t bytes, hipStream_t after);
struct GzFeed {
	GzFeedDev *d = nullptr;
	hipStream_t after = nullptr;
	template <class RT> void open(RT &rt) { d = gz_feed_open(); after = rt.stream; }
	void close() { if (d) gz_feed_close(d); d = nullptr; }
	void decode_begin(const uint8_t *src, int clen, int start_bit, const uint8_t *window, int have, int chunk_bytes, int expand) { gz_feed_decode_begin(d, src, clen, start_bit, window, have, chunk_bytes, expand); }
	void decode_end(GzLaunch &L) { gz_feed_decode_end(d, L); }
	// Two orderings that no test on a sequential double can see, both kept by events inside gz_feed_resolve_begin (GzHip::resolve_begin):
	// (i) the window may have been reallocated and copied on the feeder's stream (ensure_keep) just before: the resolve on the file's stream
	// waits for an event recorded on the feeder's stream; (ii) the feeder's stream waits for the event behind the resolve, so the parse that
	// is enqueued on it next starts only after both files' resolves (step() has also waited for both on the host by then)
	void resolve_begin(GzLaunch &L, uint8_t *text) { gz_feed_resolve_begin(d, L, text, after); }
	void resolve_end(GzLaunch &L) { gz_feed_resolve_end(d, L); }
	void decode(const uint8_t *src, int clen, int start_bit, const uint8_t *window, int have, int chunk_bytes, int expand, GzLaunch &L) { decode_begin(src, clen, start_bit, window, have, chunk_bytes, expand); decode_end(L); }
	void resolve(GzLaunch &L, uint8_t *text) { resolve_begin(L, text); resolve_end(L); }
	void upload(uint8_t *dst, const uint8_t *host, size_t bytes) { gz_feed_upload(d, dst, host, bytes, after); }
};
#else
struct GzFeed {
	std::vector<uint16_t> stage;
	std::vector<uint8_t> windows, src_;
	std::vector<GzChunk> chunks;
	GzChain chain;
	template <class RT> void open(RT &) {}
	void close() {}
	void decode_begin(const uint8_t *src, int clen, int start_bit, const uint8_t *window, int have, int chunk_bytes, int expand)
	{
		const int n = (int)(((int64_t)clen + chunk_bytes - 1) / chunk_bytes);
		src_.assign(src, src + clen);
		stage.assign((size_t)gz_stage_at(8 * (int64_t)clen, expand), 0);
		windows.assign((size_t)(n + 1) * GZ_WIN, 0);
		memcpy(windows.data(), window, GZ_WIN);
		std::vector<uint32_t> mem(GZ_WORK_BYTES / 4);
		chunks.assign((size_t)n, GzChunk());
		InfLoopDrv drv;
		GzWork w;
		gz_carve(w, (uint8_t *)mem.data());
		for (int k = 0; k < n; ++k) gz_chunk_find(drv, w, src_.data(), clen, chunk_bytes, start_bit, k, chunks[(size_t)k]);
		for (int k = 0; k < n; ++k) gz_chunk_decode(drv, w, src_.data(), clen, expand, k, n, chunks.data(), stage.data());
		gz_chain(chunks.data(), n, have, chain);
		for (int m = 0, k = 0; m < chain.n_accepted; ++m) {
			GzChunk &c = chunks[(size_t)k];
			if (c.have < GZ_WIN) for (int64_t i = 0; i < c.count; ++i) c.bad_markers += gz_bad_marker_at(stage.data() + c.stage_off, c.have, i);
			for (int i = 0; i < GZ_WIN; ++i) gz_window_at(windows.data() + (size_t)m * GZ_WIN, windows.data() + (size_t)(m + 1) * GZ_WIN, stage.data() + c.stage_off, c.count, i);
			k = c.next;
		}
	}
	void decode_end(GzLaunch &L)
	{
		L.chunks = chunks; L.chain = chain;
		for (double &u : L.us) u = 0;
	}
	void resolve_begin(GzLaunch &L, uint8_t *text)
	{
		uint32_t crc_tab[256], x2n[32];
		for (int lane = 0; lane < 64; ++lane) gz_crc_tables(crc_tab, x2n, lane, 64);
		for (GzChunk &c : L.chunks) {
			if (!(c.flags & GZ_F_ACCEPTED)) continue;
			uint8_t *out = text + c.text_off;
			for (int64_t i = 0; i < c.count; ++i) c.markers += gz_resolve_at(windows.data() + (size_t)c.order * GZ_WIN, stage.data() + c.stage_off, out, i);
			c.crc = 0;
			for (int t = 0; t < 256; ++t) c.crc ^= gz_crc_part(crc_tab, x2n, out, c.count, t, 256);
		}
	}
	void resolve_end(GzLaunch &L) { memcpy(L.window, windows.data() + (size_t)L.chain.n_accepted * GZ_WIN, GZ_WIN); }
	void decode(const uint8_t *src, int clen, int start_bit, const uint8_t *window, int have, int chunk_bytes, int expand, GzLaunch &L) { decode_begin(src, clen, start_bit, window, have, chunk_bytes, expand); decode_end(L); }
	void resolve(GzLaunch &L, uint8_t *text) { resolve_begin(L, text); resolve_end(L); }
	void upload(uint8_t *dst, const uint8_t *host, size_t bytes) { if (bytes) memcpy(dst, host, bytes); }
};
#endif

// a gzip file's raw slabs as the compressed bytes of its GzReader (hip_fqsort.h's FsGzSlabs, for the feeder's two translation units)
struct FeederGzSlabs : GzSource {
	SlabReader *rd = nullptr;
	const SlabReader::Slab *s = nullptr;
	size_t at = 0;
	bool err = false, ended = false;
	size_t read(uint8_t *to, size_t n) override
	{
		size_t got = 0;
		while (got < n && !ended) {
			if (!s) {
				s = rd->acquire();
				at = 0;
				if (!s || s->err) { err = s != nullptr; ended = true; break; }
			}
			const size_t k = n - got < s->len - at ? n - got : s->len - at;
			if (k) memcpy(to + got, s->buf + at, k);
			at += k; got += k;
			if (at == s->len) {
				if (s->eof) ended = true;
				rd->release();
				s = nullptr;
			}
		}
		return got;
	}
};

template <class RT> class DeviceFeeder : public FeederBase {
public:
	static constexpr size_t DEFAULT_CHUNK = (size_t)8 << 20, MAX_CHUNK = (size_t)256 << 20, SLAB_TARGET = (size_t)8 << 20;

	// flags: ARX_FEEDER_INFLATE_DEVICE -- a file that is BGZF is read as it is and inflated on the device; ARX_FEEDER_GUNZIP_DEVICE -- a file that
	// is ordinary gzip is (a BGZF file goes as without this flag: hip_fqsort.h's FsInput::open has the same rule)
	DeviceFeeder(int device, size_t chunk_bytes, int depth, int flags = 0) : device_(device), flags_(flags), chunk_(chunk_bytes ? chunk_bytes : DEFAULT_CHUNK), slots_((size_t)depth + 2) {}

	// ARX_OK, ARX_E_IO (a file cannot be opened) or ARX_E_DEVICE (no GPU); `error` says which
	int open(const char *r1, const char *r2)
	{
		// chunks a parse takes from each file: as many as fill SLAB_TARGET, at most 64 (ARX_FEEDER_PARSE_CHUNKS overrides: 1 makes
		// every chunk boundary a boundary between parses)
		size_t per = SLAB_TARGET / chunk_;
		per = per < 1 ? 1 : per > 64 ? 64 : per;
		if (sw_.parse_chunks) { const long v = *sw_.parse_chunks; if (v >= 1 && (size_t)v * chunk_ <= MAX_CHUNK) per = (size_t)v; }
		const char *path[2] = {r1, r2};
		// the gzip inflate's sizes (the rule is at the top of the file), inside arx_selftest_gunzip's bounds
		const int64_t gchunk = sw_.gunzip_chunk ? (int64_t)*sw_.gunzip_chunk : GZ_CHUNK_DEFAULT;
		int64_t gslab = (int64_t)chunk_ < 2 * gchunk ? 2 * gchunk : (int64_t)chunk_;
		if (gslab > GZ_SLAB_DEFAULT) gslab = GZ_SLAB_DEFAULT < 2 * gchunk ? 2 * gchunk : GZ_SLAB_DEFAULT;
		if (gslab > GZ_MAX_CHUNKS * gchunk) gslab = GZ_MAX_CHUNKS * gchunk;
		if (sw_.gunzip_slab) gslab = (int64_t)*sw_.gunzip_slab;
		if ((flags_ & ARX_FEEDER_GUNZIP_DEVICE) && (gchunk < GZ_MIN_CHUNK || gchunk > GZ_MAX_SLAB / 2 || gslab < 2 * gchunk || gslab > GZ_MAX_SLAB || gslab > GZ_MAX_CHUNKS * gchunk ||
		                                            gslab * GZ_EXPAND_DEFAULT > GZ_MAX_SYMBOLS)) {
			error = "ARX_FEEDER_GUNZIP_CHUNK / ARX_FEEDER_GUNZIP_SLAB outside the bounds of the gzip inflate";
			return ARX_E_ARG;
		}
		for (int f = 0; f < 2; ++f) { // each file by its own first bytes: R1 may be BGZF where R2 is ordinary gzip or plain text
			bool ok;
			const bool is_bgzf = file_is_bgzf(path[f]);
			bgzf_[f] = (flags_ & ARX_FEEDER_INFLATE_DEVICE) && is_bgzf;
			const bool gunzip = (flags_ & ARX_FEEDER_GUNZIP_DEVICE) && !is_bgzf && file_is_gzip(path[f]);
			if (gunzip) {
				std::unique_ptr<GzipRawReader> r(new GzipRawReader()); ok = r->open(path[f], (size_t)gslab, 1); rd_[f] = std::move(r);
				gz_[f].reset(new GzFile());
			} else if (bgzf_[f]) { std::unique_ptr<BgzfChunkReader> r(new BgzfChunkReader()); ok = r->open(path[f], chunk_, per); rd_[f] = std::move(r); }
			else { std::unique_ptr<ChunkReader> r(new ChunkReader()); ok = r->open(path[f], chunk_, per); rd_[f] = std::move(r); }
			if (!ok) { error = std::string("cannot open ") + path[f]; return ARX_E_IO; }
		}
		const std::string e = rt.init(device_);
		if (!e.empty()) { error = e; return ARX_E_DEVICE; }
		ready_ = true;
		if (sw_.times) rt.set_timing(true);
		for (int f = 0; f < 2; ++f)
			for (int i = 0; i < 2; ++i) registered_[f][i] = RT::host_register(rd_[f]->slab(i), rd_[f]->slab_cap()) == 0;
		meta_ = rt.template palloc<int32_t>(16);
		for (int f = 0; f < 2; ++f) {
			if (!gz_[f]) continue;
			rt.bind();
			gz_[f]->dev.open(rt);
			gz_[f]->src.rd = rd_[f].get();
			gz_[f]->rd.reset(new GzReader<GzFeed>(gz_[f]->dev, gz_[f]->src, gchunk, gslab, GZ_EXPAND_DEFAULT));
		}
		if (bgzf_[0] || bgzf_[1]) {
			icnt_ = rt.template palloc<int32_t>(4);
			if (posix_memalign((void **)&hcnt_, 4096, 4096)) { hcnt_ = nullptr; throw std::bad_alloc(); }
			memset(hcnt_, 0, 4096);
			hcnt_reg_ = RT::host_register(hcnt_, 4096) == 0;
		}
		for (int f = 0; f < 2; ++f) rd_[f]->start();
		return ARX_OK;
	}

	~DeviceFeeder() override
	{
		if (!ready_) return; // open() failed before the runtime was initialised: nothing on the device, the readers free their own buffers
		if (sw_.times) { // diagnostics: where the feeder thread's time went, and the kernels' own times (HIP events)
			rt.bind();
			for (auto &kv : rt.timers()) fprintf(stderr, "[arx feeder] %-16s %8.3f ms in %lld launches\n", kv.first.c_str(), kv.second.ms, (long long)kv.second.calls);
			fprintf(stderr, "[arx feeder] %lld records: waiting for the readers %.3f s, upload %.3f, line index %.3f, records %.3f, fields + scan %.3f, fill + copy home %.3f, "
			        "into the slot %.3f, carry %.3f, remainder to the next slot %.3f\n", (long long)n_records_, t_[0], t_[1], t_[2], t_[3], t_[4], t_[5], t_[6], t_[7], t_[8]);
		}
		rt.bind();
		try { rt.sync(); } catch (...) {}
		for (int f = 0; f < 2; ++f) if (gz_[f]) { try { gz_[f]->dev.close(); } catch (...) {} gz_[f]->rd.reset(); } // the device first: it waits for a launch that may still read the reader's bytes
		for (int f = 0; f < 2; ++f)
			for (int i = 0; i < 2; ++i) {
				if (registered_[f][i]) RT::host_unregister(rd_[f]->slab(i));
				rt.pfree(win_[f][i].p);
			}
		for (int f = 0; f < 2; ++f) { rt.pfree(cin_[f].p); rt.pfree(rows_[f].p); rt.pfree(ist_[f].p); }
		rt.pfree(icnt_);
		if (hcnt_) { if (hcnt_reg_) RT::host_unregister(hcnt_); free(hcnt_); }
		if (hblob_) { if (hblob_reg_) RT::host_unregister(hblob_); free(hblob_); }
		rt.pfree(cnt_.p); rt.pfree(off_.p); rt.pfree(nl_.p); rt.pfree(bmap_.p); rt.pfree(bstate_.p); rt.pfree(hdr_.p); rt.pfree(rcnt_.p); rt.pfree(roff_.p);
		rt.pfree(recl_.p); rt.pfree(tmp_.p); rt.pfree(sc_.p); rt.pfree(so_.p); rt.pfree(dvalid_.p); rt.pfree(blob_.p); rt.pfree(meta_);
		for (Slot &s : slots_) { rt.pfree(s.d_bases.p); rt.pfree(s.d_lens.p); }
	}

	int next(int64_t target_pairs, arx_super_batch *o) override
	{
		rt.bind();
		Slot &S = slots_[cur_];
		S.set_off.assign(1, 0); S.unique.clear(); S.do_rfa.clear(); S.bc_off.assign(1, 0); S.bcs.clear();
		int64_t pos = 0; // records of S already in a set
		while (pos < target_pairs || S.unique.empty()) {
			// ReadBarcodeSet on the run list: the set starts at record pos, inside runs_.front()
			int64_t n = 0;
			bool unique = false;
			enum { CAP, CHANGE, END } kind = END;
			for (;;) {
				while (runs_.size() > 1 && runs_[1].first <= pos) { runs_.pop_front(); cont_ = false; } // the run ended where the last set did
				const bool more_runs = runs_.size() > 1;
				const int64_t rem = runs_.empty() ? 0 : (more_runs ? runs_[1].first : S.n) - pos;
				const int64_t cap = cont_ ? 201 : 30000; // a set that continues the last set's barcode breaks off at its 201st record
				if (rem >= cap) { n = cap; unique = false; kind = CAP; break; }
				if (more_runs) { n = rem; unique = true; kind = CHANGE; break; }
				if (end_) { n = rem; unique = !err_; kind = END; break; }
				step(S); // the run may still continue: held back until its end, its cap or the end of the input is seen
			}
			if (n == 0) { bad_now_ = bad_base_; break; } // end of input
			const std::string &bc = runs_.front().bc;
			pos += n;
			S.set_off.push_back(pos);
			S.unique.push_back(unique);
			S.do_rfa.push_back(unique && bc.find('-') != std::string::npos && n >= 5); // worthRunningRFA
			S.bcs += bc; S.bc_off.push_back((int64_t)S.bcs.size());
			// bad_lines as the host feeder has counted them when it stops here: it has read one record past a set that ended at a
			// barcode change, none past a set that ended at a cap, everything at the end of the input
			if (kind == CAP) { cont_ = true; bad_now_ = S.badb[(size_t)pos - 1]; }
			else if (kind == CHANGE) { cont_ = false; bad_now_ = S.badb[(size_t)pos]; runs_.pop_front(); }
			else { cont_ = false; bad_now_ = bad_base_; runs_.pop_front(); }
		}
		if (S.unique.empty() && err_) { error = "read error in the FASTQ input"; return -1; }
		// what lies behind the last set opens the next super-batch: into the next slot, host and device
		Slot &T = slots_[(cur_ + 1) % slots_.size()];
		T.clear();
		T.reserve_like(S);
		ensure(T.d_bases, (size_t)S.boff.back() + (size_t)S.boff.back() / 8 + 64);
		ensure(T.d_lens, S.lens.size() + S.lens.size() / 8 + 16);
		double t0 = now();
		if (S.n > pos) append(T, S, pos, S.n);
		for (Run &r : runs_) r.first -= pos;
		S.n_out = pos; S.nb_out = S.boff[(size_t)(2 * pos)];
		rt.sync(); // the device copies are done before another stream reads the arrays
		t_[8] += now() - t0;
		memset(o, 0, sizeof *o);
		o->n_sets = (int32_t)S.unique.size(); o->n_pairs = pos; o->bad_lines = bad_now_;
		o->set_pair_off = S.set_off.data(); o->unique = S.unique.data(); o->do_rfa = S.do_rfa.data();
		o->bases = S.bases.data(); o->quals = S.quals.data(); o->lens = S.lens.data(); o->valid = S.valid.data();
		o->name_off = S.name_off.data(); o->names = S.names.data(); o->rg_off = S.rg_off.data(); o->rgs = S.rgs.data();
		o->barcode_off = S.bc_off.data(); o->barcodes = S.bcs.data();
		last_ = &S;
		cur_ = (cur_ + 1) % slots_.size();
		return o->n_sets;
	}

	int device_reads(const uint8_t **d_bases, const int32_t **d_lens, int64_t *n_bases) override
	{
		if (!last_ || !last_->n_out) return ARX_E_ARG;
		*d_bases = last_->d_bases.p; *d_lens = last_->d_lens.p; *n_bases = last_->nb_out;
		return ARX_OK;
	}

	int stats(int64_t *st) override
	{
		st[0] = n_chunks_; st[1] = n_bytes_; st[2] = n_records_; st[3] = bad_base_; st[4] = n_runs_; st[5] = 0; st[6] = n_dev_blocks_; st[7] = n_cbytes_;
		return ARX_OK;
	}

	// each file's GzReader::stats in arx_selftest_gunzip's layout, as far as the reading has come; zeros for a file the device was not given
	int gunzip_stats(int64_t *st) override
	{
		for (int f = 0; f < 2; ++f) {
			int64_t *o = st + (size_t)f * GZ_N_STATS;
			for (int k = 0; k < GZ_N_STATS; ++k) o[k] = 0;
			if (!gz_[f] || !gz_[f]->rd) continue;
			const GzReader<GzFeed> &r = *gz_[f]->rd;
			for (int k = 0; k < GZ_N_STATS; ++k) o[k] = r.stats[k];
			o[GZS_CONSUMED] = r.buf_at - r.stats[GZS_IGNORED]; o[GZS_INFLATED] = r.delivered;
			o[GZS_US_FIND] = (int64_t)r.us[0]; o[GZS_US_DECODE] = (int64_t)r.us[1]; o[GZS_US_RESOLVE] = (int64_t)(r.us[2] + r.us[3]);
		}
		return ARX_OK;
	}

private:
	static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
	double t_[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	template <class T> struct DBuf { T *p = nullptr; size_t cap = 0; };
	template <class T> void ensure(DBuf<T> &b, size_t n) // contents are not kept
	{
		if (n <= b.cap) return;
		rt.sync();
		rt.pfree(b.p); b.p = nullptr;
		b.cap = n + n / 2 + 64;
		b.p = rt.template palloc<T>(b.cap);
	}
	template <class T> void ensure_keep(DBuf<T> &b, size_t n, size_t used)
	{
		if (n <= b.cap) return;
		const size_t cap = n + n / 2 + 64;
		T *p = rt.template palloc<T>(cap);
		if (used) rt.d2d(p, b.p, used * sizeof(T));
		rt.sync();
		rt.pfree(b.p);
		b.p = p; b.cap = cap;
	}

	// one of the depth + 2 super-batches in flight.  Records [0, n) are parsed; a call of next() hands out [0, n_out) and moves the rest on.
	struct Slot {
		std::vector<int32_t> lens; std::vector<uint8_t> bases, valid; std::vector<char> quals, names, rgs;
		std::vector<int64_t> name_off, rg_off, boff, badb; // boff: 2n + 1 base offsets; badb: lines skipped (since open) before record r's header
		std::vector<int64_t> set_off, bc_off; std::vector<uint8_t> unique, do_rfa; std::string bcs;
		DBuf<uint8_t> d_bases; DBuf<int32_t> d_lens;
		int64_t n = 0, n_out = 0, nb_out = 0;
		void clear()
		{
			lens.clear(); bases.clear(); valid.clear(); quals.clear(); names.clear(); rgs.clear(); badb.clear();
			name_off.assign(1, 0); rg_off.assign(1, 0); boff.assign(1, 0);
			n = n_out = nb_out = 0;
		}
		// room for a super-batch like S's (what the last one took, and an eighth): the arrays then grow once per slot, not window by window
		void reserve_like(const Slot &S)
		{
			auto room = [](size_t n) { return n + n / 8 + 64; };
			lens.reserve(room(S.lens.size())); bases.reserve(room(S.bases.size())); quals.reserve(room(S.quals.size())); valid.reserve(room(S.valid.size()));
			names.reserve(room(S.names.size())); rgs.reserve(room(S.rgs.size())); badb.reserve(room(S.badb.size()));
			name_off.reserve(room(S.name_off.size())); rg_off.reserve(room(S.rg_off.size())); boff.reserve(room(S.boff.size()));
		}
		Slot() { clear(); }
	};
	struct Run { int64_t first; std::string bc; };

	// records [a, b) of S behind T's, host arrays and device reads
	void append(Slot &T, const Slot &S, int64_t a, int64_t b)
	{
		const int64_t b0 = S.boff[(size_t)(2 * a)], b1 = S.boff[(size_t)(2 * b)];
		append_arrays(T, b - a, S.lens.data() + 2 * a, S.bases.data() + b0, S.quals.data() + b0, b1 - b0, S.valid.data() + a,
		              S.names.data() + S.name_off[(size_t)a], S.name_off.data() + a, S.rgs.data() + S.rg_off[(size_t)a], S.rg_off.data() + a, S.badb.data() + a,
		              S.d_bases.p + b0, S.d_lens.p + 2 * a);
	}
	// n records: lens (2n), bases / quals (nb), valid (n), names / rgs with their n + 1 offsets (any origin), badb (n), and the device arrays
	void append_arrays(Slot &T, int64_t n, const int32_t *lens, const uint8_t *bases, const char *quals, int64_t nb, const uint8_t *valid, const char *names,
	                   const int64_t *name_off, const char *rgs, const int64_t *rg_off, const int64_t *badb, const uint8_t *d_bases, const int32_t *d_lens)
	{
		const int64_t at_b = T.boff.back();
		ensure_keep(T.d_bases, (size_t)(at_b + nb) + 64, (size_t)at_b);
		ensure_keep(T.d_lens, (size_t)(2 * (T.n + n)) + 16, (size_t)(2 * T.n));
		rt.d2d(T.d_bases.p + at_b, d_bases, (size_t)nb);
		rt.d2d(T.d_lens.p + 2 * T.n, d_lens, sizeof(int32_t) * (size_t)(2 * n));
		T.lens.insert(T.lens.end(), lens, lens + 2 * n);
		T.bases.insert(T.bases.end(), bases, bases + nb);
		T.quals.insert(T.quals.end(), quals, quals + nb);
		T.valid.insert(T.valid.end(), valid, valid + n);
		T.names.insert(T.names.end(), names, names + (name_off[n] - name_off[0]));
		T.rgs.insert(T.rgs.end(), rgs, rgs + (rg_off[n] - rg_off[0]));
		T.badb.insert(T.badb.end(), badb, badb + n);
		const int64_t n0 = T.name_off.back() - name_off[0], g0 = T.rg_off.back() - rg_off[0];
		for (int64_t r = 1; r <= n; ++r) { T.name_off.push_back(name_off[r] + n0); T.rg_off.push_back(rg_off[r] + g0); }
		int64_t bo = at_b;
		for (int64_t k = 0; k < 2 * n; ++k) { bo += lens[k]; T.boff.push_back(bo); }
		T.n += n;
	}

	// one more parse into S: new chunks of the file(s) that limit the common line range, then the kernels
	void step(Slot &S)
	{
		bool want[2];
		for (int f = 0; f < 2; ++f) want[f] = !eof_[f] && (lim_[f] || wlen_[f] < chunk_);
		const SlabReader::Slab *sl[2] = {nullptr, nullptr};
		double t0 = now();
		// The gzip files first, a piece of each per round, while one that wants text holds less than chunk_bytes: (1) find / decode / windows of
		// both enqueued, each on its file's stream, (2) both waited for, (3) room for both texts, (4) both resolves enqueued, (5) both waited for
		for (bool first = true;; first = false) {
			bool ask[2];
			for (int f = 0; f < 2; ++f) ask[f] = gz_[f] && want[f] && !eof_[f] && (first || wlen_[f] < chunk_);
			if (!ask[0] && !ask[1]) break;
			for (int f = 0; f < 2; ++f) if (ask[f]) gz_[f]->rd->begin();
			int64_t piece[2] = {0, 0};
			for (int f = 0; f < 2; ++f) {
				if (!ask[f]) continue;
				const int64_t k = gz_[f]->rd->next();
				if (k > 0) piece[f] = k;
				else { eof_[f] = true; if (k != GZ_END) err_ = true; } // (GZ_REWIND is never offered: can_rewind is false)
				if (gz_[f]->src.err) err_ = true; // a read error of the file is one wherever it fell: behind a member's trailer the reader sees only an end
			}
			for (int f = 0; f < 2; ++f) {
				if (!piece[f]) continue;
				if (wlen_[f] + (size_t)piece[f] >= ((size_t)1 << 30)) throw std::runtime_error("FASTQ input: a record of more than 2^30 bytes");
				ensure_keep(win_[f][wcur_[f]], wlen_[f] + (size_t)piece[f] + 64, wlen_[f]);
			}
			for (int f = 0; f < 2; ++f) if (piece[f]) gz_[f]->rd->place_begin(win_[f][wcur_[f]].p + wlen_[f]);
			for (int f = 0; f < 2; ++f) {
				if (!piece[f]) continue;
				gz_[f]->rd->place(win_[f][wcur_[f]].p + wlen_[f]);
				wlen_[f] += (size_t)piece[f]; n_bytes_ += piece[f]; ++n_chunks_;
			}
		}
		for (int f = 0; f < 2; ++f) if (want[f] && !gz_[f]) { sl[f] = rd_[f]->acquire(); if (!sl[f]) eof_[f] = true; }
		t_[0] += now() - t0; t0 = now();
		// the tables of both files' BGZF slabs go up through the runtime's page-locked staging (the stream is idle here: stage() does not wait)
		size_t row_at[2] = {0, 0}, row_bytes = 0;
		for (int f = 0; f < 2; ++f) if (sl[f] && bgzf_[f]) { row_at[f] = row_bytes; row_bytes += sl[f]->n_rows * sizeof(InfRow); }
		uint8_t *staged_rows = row_bytes ? (uint8_t *)rt.stage(row_bytes) : nullptr;
		for (int f = 0; f < 2; ++f) {
			if (!sl[f]) continue;
			const SlabReader::Slab &s = *sl[f];
			DBuf<uint8_t> &w = win_[f][wcur_[f]];
			ensure_keep(w, wlen_[f] + s.text + 64, wlen_[f]);
			if (!bgzf_[f]) { rt.h2d_staged(w.p + wlen_[f], s.buf, s.len); continue; }
			if (!s.n_rows) continue;
			// the compressed blocks and their table go up; the text appears behind the carry; the count of bad blocks comes home with the wait below
			ensure(cin_[f], s.len + 64); ensure(rows_[f], s.n_rows); ensure(ist_[f], s.n_rows);
			rt.h2d_staged(cin_[f].p, s.buf, s.len);
			memcpy(staged_rows + row_at[f], s.rows, s.n_rows * sizeof(InfRow));
			rt.h2d_staged(rows_[f].p, staged_rows + row_at[f], s.n_rows * sizeof(InfRow));
			rt.memset0(icnt_ + 2 * f, 8);
			inflate_rows(rt, cin_[f].p, (int64_t)s.len, rows_[f].p, (int)s.n_rows, w.p + wlen_[f], (int64_t)s.text, ist_[f].p, icnt_ + 2 * f);
			rt.d2h_async(hcnt_ + 2 * f, icnt_ + 2 * f, 8);
		}
		rt.sync(); // the readers may refill the buffers
		t_[1] += now() - t0;
		for (int f = 0; f < 2; ++f) {
			if (!sl[f]) continue;
			const SlabReader::Slab &s = *sl[f];
			size_t text = s.text;
			bool bad = false;
			if (bgzf_[f] && s.n_rows) {
				n_dev_blocks_ += (int64_t)s.n_rows; n_cbytes_ += (int64_t)s.len;
				if (hcnt_[2 * f] != 0) { // a block that did not inflate: the input ends in front of the first one, as at a read error of the host's inflate
					std::vector<int32_t> st(s.n_rows);
					rt.d2h(st.data(), ist_[f].p, 4 * s.n_rows);
					size_t b = 0;
					while (b < s.n_rows && st[b] == 0) ++b;
					text = b < s.n_rows ? (size_t)s.rows[b].ooff : s.text;
					bad = true;
				}
			}
			wlen_[f] += text; n_bytes_ += (int64_t)text; n_chunks_ += s.chunks;
			if (s.eof || s.err || bad) eof_[f] = true;
			if (s.err || bad) err_ = true;
			rd_[f]->release();
		}
		if (wlen_[0] >= ((size_t)1 << 30) || wlen_[1] >= ((size_t)1 << 30)) throw std::runtime_error("FASTQ input: a record of more than 2^30 bytes");
		parse_window(S);
	}

	void parse_window(Slot &S)
	{
		const int32_t n1 = (int32_t)wlen_[0], n2 = (int32_t)wlen_[1];
		FqWin w{win_[0][wcur_[0]].p, win_[1][wcur_[1]].p, n1, n2, (n1 + 15) / 16, (n2 + 15) / 16};
		const int nw = w.nw1 + w.nw2;
		int32_t L1 = 0, L2 = 0;
		double t0 = now();
		if (nw > 0) {
			ensure(cnt_, (size_t)nw + 1); ensure(off_, (size_t)nw + 2);
			rt.launch_wide("fq_nl_count", nw, KNlCount{w, cnt_.p});
			const int64_t total = rt.exclusive_scan(cnt_.p, off_.p, nw);
			rt.d2h(&L1, off_.p + w.nw1, 4);
			L2 = (int32_t)(total - L1);
			ensure(nl_, (size_t)total + 1);
			rt.launch_wide("fq_nl_fill", nw, KNlFill{w, off_.p, nl_.p});
		}
		const int32_t L = L1 < L2 ? L1 : L2;
		t_[2] += now() - t0; t0 = now();
		int32_t meta[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		int64_t n = 0;
		if (L > 0) {
			const FqLines ln{w.t1, w.t2, nl_.p, nl_.p + L1, L};
			const int nblk = (L + FQ_LINE_BLOCK - 1) / FQ_LINE_BLOCK;
			ensure(bmap_, (size_t)nblk); ensure(bstate_, (size_t)nblk); ensure(hdr_, (size_t)L); ensure(rcnt_, (size_t)nblk + 1); ensure(roff_, (size_t)nblk + 2);
			rt.launch_wide("fq_line_maps", nblk, KLineMaps{ln, bmap_.p, hdr_.p});
			rt.launch_wide("fq_line_states", 1, KLineStates{ln, bmap_.p, bstate_.p, nblk, 0, meta_});
			rt.launch_wide("fq_rec_count", nblk, KRecCount{ln, bstate_.p, hdr_.p, rcnt_.p, meta_});
			n = rt.exclusive_scan(rcnt_.p, roff_.p, nblk);
			t_[3] += now() - t0; t0 = now();
			if (n > 0) {
				const int32_t ni = (int32_t)n;
				ensure(recl_, (size_t)n); ensure(tmp_, (size_t)n); ensure(dvalid_, (size_t)n); ensure(sc_, 6 * (size_t)n + 1); ensure(so_, 6 * (size_t)n + 2);
				rt.launch_wide("fq_rec_fill", nblk, KRecFill{ln, bstate_.p, hdr_.p, roff_.p, recl_.p});
				rt.launch_wide("fq_rec_parse", ni, KRecParse{ln, recl_.p, ni, tmp_.p, sc_.p, dvalid_.p});
				rt.launch_wide("fq_run_flag", ni, KRunFlag{w.t1, tmp_.p, ni, sc_.p});
				rt.exclusive_scan(sc_.p, so_.p, 6 * ni);
				rt.launch_wide("fq_totals", 1, KTotals{so_.p, ni, meta_});
			}
			rt.d2h(meta, meta_, sizeof meta);
			t_[4] += now() - t0; t0 = now();
			if (n > 0) {
				const int32_t ni = (int32_t)n;
				const int64_t B = meta[3], N = meta[4], G = meta[5], R = meta[6], C = meta[7];
				// the blob: int32 arrays first, then the byte arrays
				const size_t o_lens = 0, o_recl = o_lens + 8 * (size_t)n, o_nlen = o_recl + 4 * (size_t)n, o_glen = o_nlen + 4 * (size_t)n, o_rfirst = o_glen + 4 * (size_t)n,
				             o_rbo = o_rfirst + 4 * (size_t)R, o_bases = o_rbo + 4 * (size_t)(R + 1), o_quals = o_bases + (size_t)B, o_names = o_quals + (size_t)B,
				             o_rgs = o_names + (size_t)N, o_valid = o_rgs + (size_t)G, o_rbc = o_valid + (size_t)n, bytes = o_rbc + (size_t)C;
				ensure(blob_, bytes + 64);
				if (bytes + 64 > hblob_cap_) {
					if (hblob_) { if (hblob_reg_) RT::host_unregister(hblob_); free(hblob_); hblob_ = nullptr; }
					hblob_cap_ = bytes + bytes / 2 + 4096;
					if (posix_memalign((void **)&hblob_, 4096, hblob_cap_)) { hblob_ = nullptr; hblob_cap_ = 0; throw std::bad_alloc(); }
					hblob_reg_ = RT::host_register(hblob_, hblob_cap_) == 0;
				}
				uint8_t *d = blob_.p;
				const FqOut fo{(int32_t *)(d + o_lens), (int32_t *)(d + o_recl), (int32_t *)(d + o_nlen), (int32_t *)(d + o_glen), (int32_t *)(d + o_rfirst), (int32_t *)(d + o_rbo),
				               d + o_bases, d + o_quals, d + o_names, d + o_rgs, d + o_valid, d + o_rbc};
				rt.launch_wide("fq_fill_reads", 2 * ni, KFillReads{ln, recl_.p, so_.p, fo});
				rt.launch_wide("fq_fill_records", ni, KFillRecords{w.t1, tmp_.p, sc_.p, so_.p, recl_.p, dvalid_.p, ni, fo});
				rt.d2h(hblob_, d, bytes);
				t_[5] += now() - t0; t0 = now();
				// into the slot
				const uint8_t *h = hblob_;
				const int32_t *recl = (const int32_t *)(h + o_recl), *nlen = (const int32_t *)(h + o_nlen), *glen = (const int32_t *)(h + o_glen);
				const int32_t *rfirst = (const int32_t *)(h + o_rfirst), *rbo = (const int32_t *)(h + o_rbo);
				hoff_n_.resize((size_t)n + 1); hoff_g_.resize((size_t)n + 1); hbad_.resize((size_t)n);
				hoff_n_[0] = hoff_g_[0] = 0;
				for (int64_t r = 0; r < n; ++r) {
					hoff_n_[(size_t)r + 1] = hoff_n_[(size_t)r] + nlen[r]; hoff_g_[(size_t)r + 1] = hoff_g_[(size_t)r] + glen[r];
					hbad_[(size_t)r] = bad_base_ + recl[r] - 4 * r; // every line before the header is a skipped one or belongs to one of the r records before
				}
				const int64_t rec0 = S.n;
				append_arrays(S, n, (const int32_t *)(h + o_lens), h + o_bases, (const char *)(h + o_quals), B, h + o_valid, (const char *)(h + o_names), hoff_n_.data(),
				              (const char *)(h + o_rgs), hoff_g_.data(), hbad_.data(), d + o_bases, (const int32_t *)(d + o_lens));
				// the run list; the first record of the parse continues the run before it if the barcodes are equal
				for (int64_t k = 0; k < R; ++k) {
					std::string bc((const char *)(h + o_rbc) + rbo[k], (size_t)(rbo[k + 1] - rbo[k]));
					if (k == 0 && have_prev_ && bc == prev_bc_) continue;
					runs_.push_back(Run{rec0 + rfirst[k], bc});
					++n_runs_;
					prev_bc_.swap(bc); have_prev_ = true;
				}
				n_records_ += n;
				t_[6] += now() - t0;
			}
		} else {
			meta[0] = 0; meta[1] = 0; meta[2] = 0;
		}
		bad_base_ += meta[2] - 4 * n;
		// a file that is read to its end and has no line left ends the input (an unterminated last line does not count, nor what the other
		// file still has); the record the end cut off is dropped
		lim_[0] = L1 == L; lim_[1] = L2 == L;
		if ((eof_[0] && lim_[0]) || (eof_[1] && lim_[1])) { end_ = true; return; }
		// carry: the bytes from the first line that was not consumed, to the front of the file's other window buffer
		t0 = now();
		for (int f = 0; f < 2; ++f) {
			const size_t from = (size_t)meta[f], left = wlen_[f] - from;
			if (!from) continue; // nothing consumed: the window stays
			DBuf<uint8_t> &to = win_[f][wcur_[f] ^ 1];
			ensure(to, left + 64);
			if (left) rt.d2d(to.p, win_[f][wcur_[f]].p + from, left);
			wcur_[f] ^= 1; wlen_[f] = left;
		}
		t_[7] += now() - t0;
	}

	RT rt;
	const FeederSwitches sw_; // read when the feeder is created (switches.h)
	int device_, flags_;
	size_t chunk_;
	std::unique_ptr<SlabReader> rd_[2];
	bool bgzf_[2] = {false, false};                 // the file's blocks are inflated on the device
	struct GzFile { GzFeed dev; FeederGzSlabs src; std::unique_ptr<GzReader<GzFeed> > rd; }; // an ordinary gzip file that the device inflates
	std::unique_ptr<GzFile> gz_[2];
	DBuf<uint8_t> cin_[2]; DBuf<InfRow> rows_[2]; DBuf<int32_t> ist_[2]; // a BGZF slab on the device: its bytes, its table, the blocks' statuses
	int32_t *icnt_ = nullptr, *hcnt_ = nullptr; bool hcnt_reg_ = false;  // per file: bad blocks, DEFLATE blocks read; device and page-locked host
	int64_t n_dev_blocks_ = 0, n_cbytes_ = 0;
	bool registered_[2][2] = {{false, false}, {false, false}};
	DBuf<uint8_t> win_[2][2]; int wcur_[2] = {0, 0}; size_t wlen_[2] = {0, 0};
	bool ready_ = false, eof_[2] = {false, false}, lim_[2] = {true, true}, end_ = false, err_ = false;
	DBuf<int32_t> cnt_, off_, nl_, rcnt_, roff_, recl_, sc_, so_;
	DBuf<uint8_t> bmap_, bstate_, hdr_, dvalid_, blob_;
	DBuf<FqRecTmp> tmp_;
	int32_t *meta_ = nullptr;
	uint8_t *hblob_ = nullptr; size_t hblob_cap_ = 0; bool hblob_reg_ = false;
	std::vector<int64_t> hoff_n_, hoff_g_, hbad_;
	std::vector<Slot> slots_; size_t cur_ = 0; Slot *last_ = nullptr;
	std::deque<Run> runs_; std::string prev_bc_; bool have_prev_ = false, cont_ = false;
	int64_t bad_base_ = 0, bad_now_ = 0, n_chunks_ = 0, n_bytes_ = 0, n_records_ = 0, n_runs_ = 0;
};

} // namespace arx

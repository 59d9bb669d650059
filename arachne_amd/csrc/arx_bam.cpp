// arx_bam.cpp -- C ABI of the BAM sink (bam_sink.h); host code only.
#include <stdio.h>
#include "bam_sink.h"
#include "bam_records.h"

extern "C" {

int arx_bam_open(const char *path, int32_t n_contigs, const char *const *names, const int32_t *lens, const char *extra_header, int32_t threads, int32_t level,
                 arx_bam **out, char *msg, int32_t msg_cap)
{
	*out = nullptr;
	arx::BamSink *w = nullptr;
	try {
		w = new arx::BamSink();
		if (!w->open(path, n_contigs, names, lens, extra_header, threads, level)) {
			if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "%s", w->error.c_str());
			delete w;
			return ARX_E_IO;
		}
	} catch (const std::exception &e) {
		if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "%s", e.what());
		delete w;
		return ARX_E_IO;
	}
	*out = (arx_bam *)w;
	return ARX_OK;
}

int arx_bam_write(arx_bam *h, const arx_bam_batch *batch)
{
	arx::BamSink *w = (arx::BamSink *)h;
	try {
		return w->write(*batch) ? ARX_OK : w->refused != ARX_OK ? w->refused : ARX_E_IO; // (refused: an indexing writer kept the batch out)
	} catch (const std::exception &e) {
		w->error = e.what();
		return ARX_E_IO;
	}
}

int arx_bam_write_select(arx_bam *h, const arx_bam_batch *batch, const int64_t *idx, int64_t n)
{
	arx::BamSink *w = (arx::BamSink *)h;
	if (n < 0 || (n > 0 && !idx)) { w->error = "bad record selection"; return ARX_E_ARG; }
	try {
		static const int64_t none = 0; // n = 0: an empty selection, not "all records"
		return w->write(*batch, idx ? idx : &none, n) ? ARX_OK : w->refused != ARX_OK ? w->refused : ARX_E_IO;
	} catch (const std::exception &e) {
		w->error = e.what();
		return ARX_E_IO;
	}
}

int arx_bam_write_encoded(arx_bam *h, const uint8_t *stream, int64_t n_bytes, int64_t n_records)
{
	arx::BamSink *w = (arx::BamSink *)h;
	try {
		return w->write_encoded(stream, n_bytes, n_records);
	} catch (const std::exception &e) {
		w->error = e.what();
		return ARX_E_IO;
	}
}

// the close of either kind of writer: the BAM first, then -- an indexing writer (arx_bam_open_indexed, arx_bgzf.hip) -- the index from the table of
// the blocks the sink recorded
int arx_bam_close_indexed(arx_bam *h, int64_t *stats, int64_t *index_stats, char *msg, int32_t msg_cap)
{
	arx::BamSink *w = (arx::BamSink *)h;
	if (index_stats) for (int k = 0; k < 20; ++k) index_stats[k] = 0;
	if (!w) return ARX_E_ARG;
	bool ok = false;
	try { ok = w->close(); } catch (const std::exception &) {}
	if (stats) { stats[0] = w->n_records; stats[1] = w->n_blocks; stats[2] = w->bytes_in; stats[3] = w->bytes_out + 28; }
	int rc = ok ? ARX_OK : ARX_E_IO;
	std::string text = ok ? std::string() : w->error;
	if (w->tap) {
		std::string err;
		int irc;
		try { irc = w->tap->finish(w->block_at, ok, index_stats, err); } catch (const std::exception &e) { irc = ARX_E_DEVICE; err = e.what(); }
		if (rc == ARX_OK && irc != ARX_OK) { rc = irc; text = err; }
	}
	if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "%s", text.c_str());
	delete w;
	return rc;
}

int arx_bam_close(arx_bam *h, int64_t *stats) { return arx_bam_close_indexed(h, stats, nullptr, nullptr, 0); }

const char *arx_bam_error(arx_bam *h) { return ((arx::BamSink *)h)->error.c_str(); }

struct RecBufHandle { arx::RecBuf buf; std::string error; };
int arx_recbuf_create(arx_recbuf **out)
{
	try { *out = (arx_recbuf *)new RecBufHandle(); } catch (const std::exception &) { *out = nullptr; return ARX_E_IO; }
	return ARX_OK;
}
int arx_recbuf_build(arx_recbuf *h, const arx_super_batch *sb, const int32_t *cand_off, const arx_cand *cands, const arx_aln *alns, const uint32_t *cigars,
                     const arx_cand_post *post, int32_t threads, arx_bam_batch *view)
{
	RecBufHandle *rb = (RecBufHandle *)h;
	if (!sb || !cand_off || !cands || !alns || !cigars || !view) { rb->error = "null argument"; return ARX_E_ARG; }
	try {
		return rb->buf.build(*sb, cand_off, cands, alns, cigars, post, threads, view, rb->error) ? ARX_OK : ARX_E_ARG;
	} catch (const std::exception &e) { rb->error = e.what(); return ARX_E_IO; }
}
int arx_recbuf_build_full(arx_recbuf *h, const arx_super_batch *sb, const int32_t *cand_off, const arx_cand *cands, const arx_aln *alns, const uint32_t *cigars,
                          const arx_cand_post *post, const arx_recbuf_full *full, int32_t threads, arx_bam_batch *view, const int32_t **bucket)
{
	RecBufHandle *rb = (RecBufHandle *)h;
	if (!sb || !cand_off || !cands || !alns || !cigars || !post || !full || !full->split || !full->tags || !full->contig_names || !full->contig_file || !view) {
		rb->error = "null argument"; return ARX_E_ARG;
	}
	if (full->chunk <= 0) { rb->error = "chunk must be positive"; return ARX_E_ARG; }
	try {
		if (!rb->buf.build(*sb, cand_off, cands, alns, cigars, post, threads, view, rb->error, full)) return ARX_E_ARG;
		if (bucket) *bucket = rb->buf.bucket.data();
		return ARX_OK;
	} catch (const std::exception &e) { rb->error = e.what(); return ARX_E_IO; }
}
int arx_bucket_table(int32_t n_contigs, const char *const *names, const int32_t *lens, int64_t chunk, int32_t *contig_file, int32_t *n_files, char *file_names,
                     int32_t cap_files, int32_t name_w)
{
	if (n_contigs < 0 || chunk <= 0 || !names || !lens || !contig_file || !n_files) return ARX_E_ARG;
	std::vector<std::string> fn;
	arx::bucket_table(n_contigs, names, lens, chunk, contig_file, fn);
	*n_files = (int32_t)fn.size();
	if (file_names) {
		if ((int64_t)fn.size() > cap_files) return ARX_E_ARG;
		for (size_t i = 0; i < fn.size(); ++i) {
			if ((int64_t)fn[i].size() + 1 > name_w) return ARX_E_ARG;
			memcpy(file_names + i * (size_t)name_w, fn[i].c_str(), fn[i].size() + 1);
		}
	}
	return ARX_OK;
}
const char *arx_recbuf_error(arx_recbuf *h) { return ((RecBufHandle *)h)->error.c_str(); }
void arx_recbuf_free(arx_recbuf *h) { delete (RecBufHandle *)h; }

}

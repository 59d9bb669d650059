// pipeline_records.h -- the records phase of a batch (arx_batch_records): the BAM-encoded primary record of every read, written in HBM by the
// functors of dev_records.h from what arx_batch_rfa (and arx_batch_post) left there plus the caller's arx_super_batch -- byte for byte what
// arx_recbuf_build -> arx_bam_write would append to a writer (bam_records.h, bam_sink.h; bamwriter.go:283-568).  Size, scan, fill; the stream
// is handed on as one block (arx_batch_records_fetch) or where it lies (arx_batch_records_view -> arx_bam_write_encoded_device).
#pragma once
#include <cstring>
#include <string>
#include "pipeline_post.h"
#include "dev_records.h"

namespace arx {

struct RecordsResult { uint8_t *d_stream = nullptr; int32_t *d_rec_off = nullptr; int64_t n_bytes = 0, n_records = 0; };

template <class RT> struct RecordsStage {
	// What the host can check before anything is launched: the super-batch is the batch's (pair count, read lengths: the qualities are read at
	// the batch's base offsets), names bam_name_ok accepts (BamSink::write's text), offsets that do not decrease.  "" or the message of ARX_E_ARG
	static std::string check(const arx_super_batch &sb, int n_reads, const int32_t *lens_host)
	{
		if (sb.n_pairs <= 0 || 2 * sb.n_pairs != (int64_t)n_reads) return "arx_batch_records: the super-batch holds " + std::to_string(sb.n_pairs) + " pairs, the batch " + std::to_string(n_reads) + " reads (2 * n_pairs must equal n_reads)";
		if (!sb.lens || !sb.quals || !sb.name_off || !sb.names || !sb.rg_off || !sb.rgs || !sb.barcode_off || !sb.barcodes || !sb.set_pair_off || !sb.unique || sb.n_sets <= 0) return "arx_batch_records: null array in the super-batch";
		if (memcmp(sb.lens, lens_host, sizeof(int32_t) * (size_t)n_reads)) return "arx_batch_records: the super-batch's read lengths are not those of the batch";
		for (int64_t p = 0; p < sb.n_pairs; ++p) {
			const int64_t ln = sb.name_off[p + 1] - sb.name_off[p];
			if (!bam_name_ok(ln)) return ARX_BAM_NAME_TEXT(2 * p);
			if (sb.rg_off[p + 1] < sb.rg_off[p] || sb.rg_off[p + 1] - sb.rg_off[p] > 65535) return "arx_batch_records: read-group offsets must not decrease (at most 65535 bytes each)";
		}
		if (sb.name_off[0] < 0 || sb.rg_off[0] < 0 || sb.barcode_off[0] < 0) return "arx_batch_records: negative offset in the super-batch";
		if (sb.set_pair_off[0] != 0 || sb.set_pair_off[sb.n_sets] != sb.n_pairs) return "arx_batch_records: set offsets must cover the super-batch";
		for (int s = 0; s < sb.n_sets; ++s) {
			if (sb.set_pair_off[s + 1] < sb.set_pair_off[s]) return "arx_batch_records: set offsets must not decrease";
			if (sb.barcode_off[s + 1] < sb.barcode_off[s] || sb.barcode_off[s + 1] - sb.barcode_off[s] > 65535) return "arx_batch_records: barcode offsets must not decrease (at most 65535 bytes each)";
		}
		return "";
	}

	// post: arx_batch_post's result for the duplicate flags, or null.  ARX_OK, or the code with its text in err.  Ends with the stream complete
	static int run(Pipeline<RT> &pipe, const typename Pipeline<RT>::DeviceBatch &b, const typename Pipeline<RT>::Work &w, const RfaResult &rfa, const PostResult *post,
	               const arx_super_batch &sb, RecordsResult &res, std::string &err)
	{
		RT &rt = pipe.rt;
		const int R = b.n_reads, NS = sb.n_sets;
		const int64_t P = sb.n_pairs;
		// the caller's arrays through the batch's staging, one block: every part on a 16-byte boundary
		auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
		const size_t n_q = (size_t)b.n_bases, n_nm = (size_t)sb.name_off[P] - (size_t)sb.name_off[0], n_rg = (size_t)sb.rg_off[P] - (size_t)sb.rg_off[0];
		const size_t n_bc = (size_t)sb.barcode_off[NS] - (size_t)sb.barcode_off[0];
		size_t at = 0;
		const size_t o_q = at; at += al(n_q);
		const size_t o_nm = at; at += al(n_nm);
		const size_t o_rg = at; at += al(n_rg);
		const size_t o_bc = at; at += al(n_bc);
		const size_t o_bx = at; at += al((size_t)NS);
		const size_t o_no = at; at += al(8 * ((size_t)P + 1));
		const size_t o_ro = at; at += al(8 * ((size_t)P + 1));
		const size_t o_bo = at; at += al(8 * ((size_t)NS + 1));
		const size_t o_so = at; at += al(8 * ((size_t)NS + 1));
		uint8_t *st = (uint8_t *)rt.stage(at + 16);
		if (n_q) memcpy(st + o_q, sb.quals, n_q);
		memcpy(st + o_nm, sb.names + sb.name_off[0], n_nm);
		if (n_rg) memcpy(st + o_rg, sb.rgs + sb.rg_off[0], n_rg);
		if (n_bc) memcpy(st + o_bc, sb.barcodes + sb.barcode_off[0], n_bc);
		for (int s = 0; s < NS; ++s) st[o_bx + s] = bam_set_bx(sb.unique[s], sb.barcodes + sb.barcode_off[s], sb.barcode_off[s + 1] - sb.barcode_off[s]);
		int64_t *no = (int64_t *)(st + o_no), *ro = (int64_t *)(st + o_ro), *bo = (int64_t *)(st + o_bo);
		for (int64_t p = 0; p <= P; ++p) { no[p] = sb.name_off[p] - sb.name_off[0]; ro[p] = sb.rg_off[p] - sb.rg_off[0]; }
		for (int s = 0; s <= NS; ++s) bo[s] = sb.barcode_off[s] - sb.barcode_off[0];
		memcpy(st + o_so, sb.set_pair_off, 8 * ((size_t)NS + 1));
		uint8_t *d_in = rt.template alloc<uint8_t>(at + 16);
		rt.h2d_staged(d_in, st, at);
		RecInputs in;
		in.quals = d_in + o_q; in.names = d_in + o_nm; in.name_off = (const int64_t *)(d_in + o_no); in.rgs = d_in + o_rg; in.rg_off = (const int64_t *)(d_in + o_ro);
		in.barcodes = d_in + o_bc; in.barcode_off = (const int64_t *)(d_in + o_bo); in.set_pair_off = (const int64_t *)(d_in + o_so); in.set_bx = d_in + o_bx; in.n_sets = NS;

		RecMeta *meta = rt.template alloc<RecMeta>((size_t)R + 1);
		int32_t *size = rt.template alloc<int32_t>((size_t)R + 1), *rec_off = rt.template alloc<int32_t>((size_t)R + 2);
		uint32_t *d_err = rt.template alloc<uint32_t>(4);
		rt.memset0(d_err, 16);
		KBamRecSize ks{rfa.d_cands, rfa.d_cand_off, w.c_alns, w.c_cig, post ? post->d_post : nullptr, b.lens, b.base_off, in, meta, size, d_err};
		rt.launch_wide("rec_size", R, ks);
		const int64_t total = rt.exclusive_scan(size, rec_off, R);
		uint32_t e = 0;
		rt.d2h(&e, d_err, 4);
		if (e & REC_ERR_NO_ACTIVE) { err = "a read without an active candidate: arx_batch_rfa must have run on this batch"; return ARX_E_ARG; }
		if (total >= ((int64_t)1 << 31) - 1) { err = "batch too large: more than 2^31 bytes of BAM records, split the batch"; return ARX_E_TOO_LARGE; }
		const int n_words = (int)((total + 15) / 16), n_tiles = (int)((total + REC_TILE - 1) / REC_TILE);
		int32_t *tile_first = rt.template alloc<int32_t>((size_t)n_tiles + 1);
		RecWord16 *stream = rt.template alloc<RecWord16>((size_t)n_words + 1);
		KBamRecTile kt{rec_off, R, tile_first};
		rt.launch_wide("rec_tile", n_tiles, kt);
		KBamRecFill kf{RecSources{w.c_cig, b.bases, in}, meta, rec_off, tile_first, R, total, stream};
		rt.launch_wide("rec_fill", n_words, kf);
		rt.sync();
		res.d_stream = (uint8_t *)stream; res.d_rec_off = rec_off; res.n_bytes = total; res.n_records = R;
		return ARX_OK;
	}
	// the stream as one block; rec_off (may be null): n_records + 1 byte offsets
	static void fetch(Pipeline<RT> &pipe, const RecordsResult &res, uint8_t *stream, int64_t *rec_off)
	{
		RT &rt = pipe.rt;
		if (stream) rt.d2h(stream, res.d_stream, (size_t)res.n_bytes);
		if (rec_off) {
			std::vector<int32_t> o((size_t)res.n_records + 1);
			rt.d2h(o.data(), res.d_rec_off, 4 * o.size());
			for (size_t i = 0; i < o.size(); ++i) rec_off[i] = o[i];
		}
	}
};

} // namespace arx

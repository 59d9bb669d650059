// pipeline_records.h -- the records phase of a batch (arx_batch_records): the BAM-encoded primary record of every read, written in HBM by the
// functors of dev_records.h from what arx_batch_rfa (and arx_batch_post) left there plus the caller's arx_super_batch -- byte for byte what
// arx_recbuf_build -> arx_bam_write would append to a writer (bam_records.h, bam_sink.h; bamwriter.go:283-568).  Size, scan, fill; the stream
// is handed on as one block (arx_batch_records_fetch) or where it lies (arx_batch_records_view -> arx_bam_write_encoded_device).
// RecordsFullStage (arx_batch_records_full) is the same phase for the reference's record set and its position buckets (dev_records_full.h).
#pragma once
#include <cstring>
#include <string>
#include <vector>
#include "pipeline_post.h"
#include "dev_records.h"
#include "dev_records_full.h"

namespace arx {

struct RecordsResult {
	uint8_t *d_stream = nullptr; int32_t *d_rec_off = nullptr; int64_t n_bytes = 0, n_records = 0;
	// arx_batch_records_full only (full): the records' buckets, the stream grouped by bucket and where each bucket starts in it
	bool full = false; int32_t n_files = 0; int32_t *d_bucket = nullptr; uint8_t *d_grouped = nullptr; std::vector<int64_t> bucket_byte_off, bucket_rec_off;
};

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

	// the caller's arrays through the batch's staging into device memory, one block, every part on a 16-byte boundary (extra: n_extra more
	// words behind them, the full phase's contig_file)
	static RecInputs upload(Pipeline<RT> &pipe, const typename Pipeline<RT>::DeviceBatch &b, const arx_super_batch &sb, const int32_t *extra, int n_extra, const int32_t **d_extra)
	{
		RT &rt = pipe.rt;
		const int NS = sb.n_sets;
		const int64_t P = sb.n_pairs;
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
		const size_t o_ex = at; at += al(4 * (size_t)n_extra);
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
		if (n_extra) memcpy(st + o_ex, extra, 4 * (size_t)n_extra);
		uint8_t *d_in = rt.template alloc<uint8_t>(at + 16);
		rt.h2d_staged(d_in, st, at);
		RecInputs in;
		in.quals = d_in + o_q; in.names = d_in + o_nm; in.name_off = (const int64_t *)(d_in + o_no); in.rgs = d_in + o_rg; in.rg_off = (const int64_t *)(d_in + o_ro);
		in.barcodes = d_in + o_bc; in.barcode_off = (const int64_t *)(d_in + o_bo); in.set_pair_off = (const int64_t *)(d_in + o_so); in.set_bx = d_in + o_bx; in.n_sets = NS;
		if (d_extra) *d_extra = (const int32_t *)(d_in + o_ex);
		return in;
	}

	// post: arx_batch_post's result for the duplicate flags, or null.  ARX_OK, or the code with its text in err.  Ends with the stream complete
	static int run(Pipeline<RT> &pipe, const typename Pipeline<RT>::DeviceBatch &b, const typename Pipeline<RT>::Work &w, const RfaResult &rfa, const PostResult *post,
	               const arx_super_batch &sb, RecordsResult &res, std::string &err)
	{
		RT &rt = pipe.rt;
		const int R = b.n_reads;
		const RecInputs in = upload(pipe, b, sb, nullptr, 0, nullptr);

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
		res = RecordsResult();
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

// arx_batch_records_full: the reference's record set (DoDumpToBam, bamwriter.go:278-566, 635-689) by the functors of dev_records_full.h, and
// the same records grouped by position bucket (AppendBams, :279-281; the files of CreateBAMs, :134-188).  Needs the post and the tags phase
template <class RT> struct RecordsFullStage {
	static std::string check_layout(const arx_records_layout *lay, int n_contigs)
	{
		if (!lay || !lay->contig_file) return "arx_batch_records_full: null layout";
		if (lay->n_contigs != n_contigs) return "arx_batch_records_full: the layout has " + std::to_string(lay->n_contigs) + " contigs, the index " + std::to_string(n_contigs);
		if (lay->chunk <= 0 || lay->unmapped_file < 0) return "arx_batch_records_full: chunk must be positive and unmapped_file the last file of arx_bucket_table";
		if ((int64_t)lay->unmapped_file + 1 > REC_MAX_FILES) return "arx_batch_records_full: " + std::to_string((int64_t)lay->unmapped_file + 1) + " files, the grouping holds at most " + std::to_string(REC_MAX_FILES) + " (use a larger chunk)";
		for (int i = 0; i < n_contigs; ++i) if (lay->contig_file[i] < 0 || lay->contig_file[i] >= lay->unmapped_file) return "arx_batch_records_full: contig_file is not arx_bucket_table's (a file outside [0, unmapped_file))";
		return "";
	}
	// d_names / d_name_off: the context's contig names in device memory.  ARX_OK, or the code with its text in err.  Ends with both streams complete
	static int run(Pipeline<RT> &pipe, const typename Pipeline<RT>::DeviceBatch &b, const typename Pipeline<RT>::Work &w, const RfaResult &rfa, const PostResult &post,
	               const TagsResult &tags, const arx_super_batch &sb, const arx_records_layout &lay, const uint8_t *d_names, const int32_t *d_name_off, RecordsResult &res, std::string &err)
	{
		RT &rt = pipe.rt;
		const int R = b.n_reads, NF = lay.unmapped_file + 1;
		const int32_t *d_contig_file = nullptr;
		const RecInputs in = RecordsStage<RT>::upload(pipe, b, sb, lay.contig_file, lay.n_contigs, &d_contig_file);
		// the text of every mismatch entry
		const int64_t NM = post.n_mm;
		int32_t *mm_len = rt.template alloc<int32_t>((size_t)NM + 1), *mm_txt_off = rt.template alloc<int32_t>((size_t)NM + 2);
		if (NM > 0) {
			KRecMmLen km{post.d_mm_ref, post.d_mm_read, mm_len};
			rt.launch_wide("rec_mm_len", (int)NM, km);
			if (rt.exclusive_scan(mm_len, mm_txt_off, (int)NM) >= ((int64_t)1 << 31) - 1) { err = "batch too large: more than 2^31 bytes of mismatch text, split the batch"; return ARX_E_TOO_LARGE; }
		} else rt.memset0(mm_txt_off, 8);
		RecFullInputs F;
		F.post = post.d_post; F.split = post.d_split; F.tags = tags.d_tags; F.mm_ref = post.d_mm_ref; F.mm_read = post.d_mm_read; F.mm_txt_off = mm_txt_off;
		F.contig_names = d_names; F.contig_name_off = d_name_off; F.contig_file = d_contig_file; F.n_contigs = lay.n_contigs; F.unmapped_file = lay.unmapped_file; F.chunk = lay.chunk;
		// records per read, then per record its meta, size and bucket
		int32_t *n_rec = rt.template alloc<int32_t>((size_t)R + 1), *rbase = rt.template alloc<int32_t>((size_t)R + 2);
		uint32_t *d_err = rt.template alloc<uint32_t>(4);
		rt.memset0(d_err, 16);
		KRecFullCount kc{rfa.d_cands, rfa.d_cand_off, post.d_split, n_rec, d_err};
		rt.launch_wide("rec_full_count", R, kc);
		const int64_t NRec = rt.exclusive_scan(n_rec, rbase, R);
		uint32_t e = 0;
		rt.d2h(&e, d_err, 4);
		if (e & REC_ERR_NO_ACTIVE) { err = "a read without an active candidate: arx_batch_rfa must have run on this batch"; return ARX_E_ARG; }
		if (e & REC_ERR_SPLIT) { err = ARX_BAM_SPLIT_TEXT; return ARX_E_ARG; }
		RecFullMeta *meta = rt.template alloc<RecFullMeta>((size_t)NRec + 1);
		int32_t *size = rt.template alloc<int32_t>((size_t)NRec + 1), *bucket = rt.template alloc<int32_t>((size_t)NRec + 1), *rec_off = rt.template alloc<int32_t>((size_t)NRec + 2);
		KRecFullMeta km{rfa.d_cands, rfa.d_cand_off, w.c_alns, w.c_cig, b.lens, b.base_off, in, F, rbase, meta, size, bucket, d_err};
		rt.launch_wide("rec_full_meta", R, km);
		const int64_t total = rt.exclusive_scan(size, rec_off, (int)NRec);
		rt.d2h(&e, d_err, 4);
		if (e & REC_ERR_BUCKET) { err = "arx_batch_records_full: a record's bucket lies outside the table: contig_file / chunk are not arx_bucket_table's for this index"; return ARX_E_ARG; }
		if (total >= ((int64_t)1 << 31) - 1) { err = "batch too large: more than 2^31 bytes of BAM records, split the batch"; return ARX_E_TOO_LARGE; }
		// the grouping's table (dev_records_full.h: KRecGroupCount), refused before the first fill is queued
		const int NB = (int)((NRec + REC_GROUP_BLOCK - 1) / REC_GROUP_BLOCK);
		const int64_t n_tab = (int64_t)NF * NB;
		if (n_tab > REC_MAX_GROUP_TABLE) { err = "batch too large: the grouping table of " + std::to_string(NF) + " files x " + std::to_string(NB) + " blocks of records exceeds " + std::to_string(REC_MAX_GROUP_TABLE) + " entries, split the batch or use a larger chunk"; return ARX_E_TOO_LARGE; }
		const int n_words = (int)((total + 15) / 16), n_tiles = (int)((total + REC_TILE - 1) / REC_TILE);
		const RecFullSources S{w.c_cig, b.bases, in, F};
		int32_t *tile_first = rt.template alloc<int32_t>((size_t)n_tiles + 1);
		RecWord16 *stream = rt.template alloc<RecWord16>((size_t)n_words + 1);
		KBamRecTile kt{rec_off, (int)NRec, tile_first};
		rt.launch_wide("rec_tile", n_tiles, kt);
		KRecFullFill kf{S, meta, nullptr, rec_off, tile_first, (int)NRec, total, stream};
		rt.launch_wide("rec_full_fill", n_words, kf);
		// the stable order by bucket (dev_records_full.h: KRecGroupCount) and the grouped stream: the same fill over the permuted order
		int32_t *cnt = rt.template alloc<int32_t>((size_t)n_tab + 1), *base = rt.template alloc<int32_t>((size_t)n_tab + 2);
		int32_t *order = rt.template alloc<int32_t>((size_t)NRec + 1), *gsize = rt.template alloc<int32_t>((size_t)NRec + 1), *g_off = rt.template alloc<int32_t>((size_t)NRec + 2);
		int64_t *d_boff = rt.template alloc<int64_t>(2 * ((size_t)NF + 1));
		rt.memset0(cnt, 4 * (size_t)n_tab);
		KRecGroupCount gc{bucket, (int)NRec, NB, cnt};
		rt.launch_wide("rec_group_count", NB, gc);
		rt.exclusive_scan(cnt, base, (int)n_tab);
		rt.memset0(cnt, 4 * (size_t)n_tab);
		KRecGroupRank gr{bucket, base, (int)NRec, NB, cnt, order};
		rt.launch_wide("rec_group_rank", NB, gr);
		KRecGroupSize gs{size, order, gsize};
		rt.launch_wide("rec_group_size", (int)NRec, gs);
		rt.exclusive_scan(gsize, g_off, (int)NRec);
		KRecGroupOff go{base, g_off, NF, NB, (int)NRec, d_boff, d_boff + NF + 1};
		rt.launch_wide("rec_group_off", NF + 1, go);
		int32_t *g_tile = rt.template alloc<int32_t>((size_t)n_tiles + 1);
		RecWord16 *grouped = rt.template alloc<RecWord16>((size_t)n_words + 1);
		KBamRecTile gt{g_off, (int)NRec, g_tile};
		rt.launch_wide("rec_tile", n_tiles, gt);
		KRecFullFill gf{S, meta, order, g_off, g_tile, (int)NRec, total, grouped};
		rt.launch_wide("rec_full_fill", n_words, gf);
		res = RecordsResult();
		res.bucket_rec_off.resize((size_t)NF + 1); res.bucket_byte_off.resize((size_t)NF + 1);
		rt.d2h(res.bucket_rec_off.data(), d_boff, 8 * ((size_t)NF + 1));
		rt.d2h(res.bucket_byte_off.data(), d_boff + NF + 1, 8 * ((size_t)NF + 1));
		rt.sync();
		res.d_stream = (uint8_t *)stream; res.d_rec_off = rec_off; res.n_bytes = total; res.n_records = NRec;
		res.full = true; res.n_files = NF; res.d_bucket = bucket; res.d_grouped = (uint8_t *)grouped;
		return ARX_OK;
	}
	// any of the four may be null
	static void fetch_buckets(Pipeline<RT> &pipe, const RecordsResult &res, int32_t *bucket, uint8_t *grouped, int64_t *bucket_byte_off, int64_t *bucket_rec_off)
	{
		RT &rt = pipe.rt;
		if (bucket) rt.d2h(bucket, res.d_bucket, 4 * (size_t)res.n_records);
		if (grouped) rt.d2h(grouped, res.d_grouped, (size_t)res.n_bytes);
		if (bucket_byte_off) memcpy(bucket_byte_off, res.bucket_byte_off.data(), 8 * res.bucket_byte_off.size());
		if (bucket_rec_off) memcpy(bucket_rec_off, res.bucket_rec_off.data(), 8 * res.bucket_rec_off.size());
	}
};

} // namespace arx

// bam_sink.h -- the BAM sink behind the path, host code of libarachne_amd.so.
//
// What it replaces: the reference funnels every record of every barcode through ONE goroutine (BamThread, bamwriter.go:615-627) that
// builds a biogo sam.Record per alignment and writes it twice (AppendBams :279-282: the barcode-sorted BAM and a position bucket), each
// bam.Writer compressing with two BGZF goroutines (bam.NewWriter(file, h, 2), :118).  At a few hundred thousand records per second that
// caps the program far below what the GPU path delivers.  Here a writer takes records in BATCHES as flat arrays (what AppendBam
// computes per alignment -- name, flags, reference, position, MAPQ, CIGAR, mate, template length, bases, qualities, aux bytes -- stays
// the caller's business), encodes them into the BAM byte stream in parallel (record sizes -> prefix sums -> every thread fills its
// slice), cuts the stream into BGZF blocks and deflates the blocks on `threads` host threads; blocks reach the file in order.
//
// Format: SAM/BAM specification v1 (magic BAM\1, header text, references, records with bin from reg2bin, 4-bit bases, BGZF blocks of at
// most 65280 input bytes with the BC extra field, the 28-byte EOF block).  The bytes of the DEFLATE streams depend on the compressor
// (biogo/hts v1.4.5 uses Go's compress/gzip, this uses zlib): "byte-identical to the reference's file" is not a property any BAM writer
// can be held to; what is checked (tests/test_bam_sink.py) is that the decompressed stream is exactly the specified encoding of the
// records handed in.  The reference's library is absent from /root/reference (go.mod:5), so that is the pin: parity unpinned by it.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include "../../include/arachne_amd.h"
#include "bam_rules.h"

namespace arx {

// The seam behind flush(): something else that turns `total` bytes, cut every BamSink::BLOCK_IN bytes, into framed BGZF blocks and writes them to f
// in order, adding what it wrote to bytes_out.  BamSink's own path (zlib on `threads` host threads) is the default; hip_bgzf.h holds the one
// that compresses on the GPU (arx_bam_open_device).  sizes: null, or where the framed size of every block written is appended, in order (a writer
// that records where its blocks lie: BamSink::record_blocks).
struct BlockCompressor {
	virtual ~BlockCompressor() {}
	virtual bool run(const uint8_t *src, size_t total, FILE *f, int64_t &bytes_out, std::string &error, std::vector<int64_t> *sizes) = 0;
};

// What an indexing writer (arx_bam_open_indexed; arx_bgzf.hip holds the one implementation) hangs on its sink: it is shown every append before
// the sink takes it, and is handed the table of the blocks once the file is closed.
struct StreamTap {
	virtual ~StreamTap() {}
	// p[0, n): the next bytes of the record stream, in host memory (device < 0) or in the memory of that HIP device.  ARX_OK: the sink goes on
	// and appends them; anything else: it appends nothing, error says why
	virtual int take(const uint8_t *p, int64_t n, int device, std::string &error) = 0;
	// the file is closed: block_at[0 .. n_blocks], the last entry the EOF block's.  bam_ok: every append and the close went well
	virtual int finish(const std::vector<int64_t> &block_at, bool bam_ok, int64_t *index_stats, std::string &error) = 0;
};

struct BamSink {
	FILE *f = nullptr;
	std::shared_ptr<BlockCompressor> comp; // null: deflate_block below
	int threads = 1, level = 6;
	bool coordinate = false;               // set before open(): @HD says SO:coordinate (arx_bam_open_ex; what is appended is the caller's to order)
	std::string error;
	std::vector<uint8_t> pending;         // uncompressed bytes not yet cut into a block
	int64_t n_records = 0, n_blocks = 0, bytes_in = 0, bytes_out = 0;
	bool record_blocks = false;           // set before open(): block_at keeps the file offset of every block written (8 bytes a block), the EOF block's last
	std::vector<int64_t> block_at;
	std::unique_ptr<StreamTap> tap;       // null: a plain writer
	int refused = ARX_OK;                 // what the tap answered where it kept the last append out
	static constexpr size_t BLOCK_IN = 0xff00; // BGZF: at most 64 KiB per block after compression; 65280 input bytes always fit

	static void put32(std::vector<uint8_t> &v, uint32_t x) { for (int i = 0; i < 4; ++i) v.push_back((uint8_t)(x >> (8 * i))); }
	static void w32(uint8_t *p, uint32_t x) { p[0] = (uint8_t)x; p[1] = (uint8_t)(x >> 8); p[2] = (uint8_t)(x >> 16); p[3] = (uint8_t)(x >> 24); }
	static void w16(uint8_t *p, uint32_t x) { p[0] = (uint8_t)x; p[1] = (uint8_t)(x >> 8); }

	bool open(const char *path, int n_contigs, const char *const *names, const int32_t *lens, const char *extra_header, int threads_, int level_)
	{
		f = fopen(path, "wb");
		if (!f) { error = std::string("cannot write ") + path; return false; }
		threads = threads_ > 0 ? threads_ : 1;
		level = level_ >= 0 && level_ <= 9 ? level_ : 6;
		std::string text = coordinate ? "@HD\tVN:1.6\tSO:coordinate\n" : "@HD\tVN:1.6\tSO:unknown\n";
		for (int i = 0; i < n_contigs; ++i) text += std::string("@SQ\tSN:") + names[i] + "\tLN:" + std::to_string(lens[i]) + "\n";
		if (extra_header) text += extra_header;
		std::vector<uint8_t> h;
		h.push_back('B'); h.push_back('A'); h.push_back('M'); h.push_back(1);
		put32(h, (uint32_t)text.size());
		h.insert(h.end(), text.begin(), text.end());
		put32(h, (uint32_t)n_contigs);
		for (int i = 0; i < n_contigs; ++i) {
			const size_t l = strlen(names[i]) + 1;
			put32(h, (uint32_t)l);
			h.insert(h.end(), names[i], names[i] + l);
			put32(h, (uint32_t)lens[i]);
		}
		pending = h;
		return flush(true); // the header ends its own block(s), as htslib and biogo write it
	}

	static uint8_t base4(uint8_t c)
	{
		switch (c) { // "=ACMGRSVTWYHKDBN"
		case '=': return 0; case 'A': case 'a': return 1; case 'C': case 'c': return 2; case 'M': case 'm': return 3; case 'G': case 'g': return 4;
		case 'R': case 'r': return 5; case 'S': case 's': return 6; case 'V': case 'v': return 7; case 'T': case 't': return 8; case 'W': case 'w': return 9;
		case 'Y': case 'y': return 10; case 'H': case 'h': return 11; case 'K': case 'k': return 12; case 'D': case 'd': return 13; case 'B': case 'b': return 14;
		default: return 15;
		}
	}

	static size_t record_size(const arx_bam_batch &b, int64_t i)
	{
		const size_t l_name = (size_t)(b.name_off[i + 1] - b.name_off[i]) + 1, n_cig = (size_t)(b.cigar_off[i + 1] - b.cigar_off[i]);
		const size_t l_seq = (size_t)(b.seq_off[i + 1] - b.seq_off[i]), l_aux = (size_t)(b.aux_off[i + 1] - b.aux_off[i]);
		return 4 + 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq + l_aux;
	}
	static void encode(const arx_bam_batch &b, int64_t i, uint8_t *p)
	{
		const size_t sz = record_size(b, i);
		const size_t l_name = (size_t)(b.name_off[i + 1] - b.name_off[i]) + 1, n_cig = (size_t)(b.cigar_off[i + 1] - b.cigar_off[i]);
		const size_t l_seq = (size_t)(b.seq_off[i + 1] - b.seq_off[i]), l_aux = (size_t)(b.aux_off[i + 1] - b.aux_off[i]);
		const uint32_t *cg = b.cigars + b.cigar_off[i];
		uint32_t fixed[9];
		bam_fixed(fixed, (int64_t)sz, b.rid[i], b.pos[i], (uint8_t)l_name, b.mapq[i], bam_bin(b.pos[i], bam_ref_len(cg, (int)n_cig, false)), (uint32_t)n_cig, (uint32_t)b.flag[i], (uint32_t)l_seq,
		          b.mate_rid[i], b.mate_pos[i], b.tlen[i]);
		for (int k = 0; k < 9; ++k) w32(p + 4 * k, fixed[k]);
		uint8_t *q = p + 36;
		memcpy(q, b.names + b.name_off[i], l_name - 1); q[l_name - 1] = 0; q += l_name;
		for (size_t k = 0; k < n_cig; ++k) w32(q + 4 * k, cg[k]);
		q += 4 * n_cig;
		const uint8_t *s = b.seq + b.seq_off[i];
		for (size_t k = 0; k + 1 < l_seq; k += 2) *q++ = (uint8_t)(base4(s[k]) << 4 | base4(s[k + 1]));
		if (l_seq & 1) *q++ = (uint8_t)(base4(s[l_seq - 1]) << 4);
		const uint8_t *ql = b.qual + b.seq_off[i];
		if (b.qual_offset == 255) memset(q, 0xff, l_seq); // no qualities
		else for (size_t k = 0; k < l_seq; ++k) q[k] = (uint8_t)(ql[k] - b.qual_offset);
		q += l_seq;
		if (l_aux) memcpy(q, b.aux + b.aux_off[i], l_aux);
	}

	template <class F> void parallel(size_t n, F fn)
	{
		const int T = (int)(n < (size_t)threads ? (n ? n : 1) : threads);
		if (T <= 1) { fn(0, n); return; }
		std::vector<std::thread> th;
		for (int t = 0; t < T; ++t) th.emplace_back([=]() { fn(n * t / T, n * (t + 1) / T); });
		for (auto &x : th) x.join();
	}

	// idx: the records to write, in this order (arx_bam_write_select), or null for all of them
	bool write(const arx_bam_batch &b, const int64_t *idx = nullptr, int64_t n_sel = 0)
	{
		const int64_t n = idx ? n_sel : b.n_records;
		auto rec = [&](int64_t k) { return idx ? idx[k] : k; };
		refused = ARX_OK;
		for (int64_t k = 0; k < n; ++k) {
			const int64_t i = rec(k);
			if (i < 0 || i >= b.n_records) { error = "record index " + std::to_string(i) + " outside the batch"; return false; }
			const int64_t ln = b.name_off[i + 1] - b.name_off[i], nc = b.cigar_off[i + 1] - b.cigar_off[i];
			if (!bam_name_ok(ln)) { error = ARX_BAM_NAME_TEXT(i); return false; }
			if (nc < 0 || nc > 65535) { error = "record " + std::to_string(i) + " has more than 65535 CIGAR operations"; return false; }
		}
		std::vector<size_t> off((size_t)n + 1, 0);
		for (int64_t k = 0; k < n; ++k) off[k + 1] = off[k] + record_size(b, rec(k));
		const size_t base = pending.size();
		pending.resize(base + off[n]);
		uint8_t *dst = pending.data() + base;
		parallel((size_t)n, [&](size_t lo, size_t hi) { for (size_t k = lo; k < hi; ++k) encode(b, rec((int64_t)k), dst + off[k]); });
		if (admit(dst, (int64_t)off[n], -1) != ARX_OK) { pending.resize(base); return false; } // (encoded where they would lie: nothing of them stays)
		n_records += n;
		return flush(false);
	}

	// The one hand-over: every append shows its bytes to the tap first, where there is one, and only then reaches the sink (put_raw, the device
	// sink's run_device, or write() above, which encodes in place).  device: where p lies (StreamTap::take).  Not ARX_OK: nothing is to be appended
	int admit(const uint8_t *p, int64_t n, int device)
	{
		refused = ARX_OK;
		if (!tap || n <= 0) return ARX_OK;
		return refused = tap->take(p, n, device, error);
	}
	// n admitted bytes of host memory behind what is pending
	bool put_raw(const uint8_t *p, size_t n, int64_t recs)
	{
		pending.insert(pending.end(), p, p + n);
		n_records += recs;
		return flush(false);
	}
	// the file offset of the next block written, where the writer records them
	void note_blocks(const std::vector<int64_t> &sizes, int64_t from)
	{
		for (int64_t z : sizes) { block_at.push_back(from); from += z; }
	}

	// arx_bam_write_encoded: records that are BAM-encoded already (what encode() writes, e.g. by the device: dev_records.h).  Checked is only what is
	// cheap: the block_size fields must tile n_bytes into exactly n records of at least the fixed part.  ARX_OK, ARX_E_ARG (nothing appended) or ARX_E_IO
	static uint32_t r32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
	int write_encoded(const uint8_t *stream, int64_t n_bytes, int64_t n)
	{
		if (n_bytes < 0 || n < 0 || (n_bytes > 0 && !stream)) { error = "arx_bam_write_encoded: bad arguments"; return ARX_E_ARG; }
		int64_t at = 0, seen = 0;
		while (at < n_bytes) {
			const int64_t left = n_bytes - at;
			const int64_t bs = left >= 4 ? (int64_t)r32(stream + at) : -1;
			if (bs < 32 || bs > left - 4) { error = "arx_bam_write_encoded: the block_size fields do not tile the stream (record " + std::to_string(seen) + " at byte " + std::to_string(at) + ")"; return ARX_E_ARG; }
			at += 4 + bs; ++seen;
		}
		if (seen != n) { error = "arx_bam_write_encoded: the stream holds " + std::to_string(seen) + " records, not " + std::to_string(n); return ARX_E_ARG; }
		const int rc = admit(stream, n_bytes, -1);
		if (rc != ARX_OK) return rc;
		return put_raw(stream, (size_t)n_bytes, n) ? ARX_OK : ARX_E_IO;
	}

	// compresses every whole block of `pending` (all of it when `all`), writes them in order
	bool flush(bool all)
	{
		const size_t total = pending.size();
		const size_t nb = all ? (total + BLOCK_IN - 1) / BLOCK_IN : total / BLOCK_IN;
		if (nb == 0) return true;
		if (comp) {
			const size_t used = all ? total : nb * BLOCK_IN;
			std::vector<int64_t> sizes;
			const int64_t from = bytes_out;
			if (!comp->run(pending.data(), used, f, bytes_out, error, record_blocks ? &sizes : nullptr)) return false;
			if (record_blocks) {
				if (sizes.size() != nb) { error = "the compressor reported the sizes of " + std::to_string(sizes.size()) + " blocks, not " + std::to_string(nb); return false; }
				note_blocks(sizes, from);
			}
			n_blocks += (int64_t)nb; bytes_in += (int64_t)used;
			pending.erase(pending.begin(), pending.begin() + used);
			return true;
		}
		std::vector<std::vector<uint8_t> > out(nb);
		std::vector<int> ok(nb, 1);
		parallel(nb, [&](size_t lo, size_t hi) {
			for (size_t k = lo; k < hi; ++k) {
				const size_t b0 = k * BLOCK_IN, len = (b0 + BLOCK_IN <= total) ? BLOCK_IN : total - b0;
				ok[k] = deflate_block(pending.data() + b0, len, out[k]) ? 1 : 0;
			}
		});
		for (size_t k = 0; k < nb; ++k) {
			if (!ok[k]) { error = "deflate failed"; return false; }
			if (fwrite(out[k].data(), 1, out[k].size(), f) != out[k].size()) { error = "write failed"; return false; }
			if (record_blocks) block_at.push_back(bytes_out);
			bytes_out += (int64_t)out[k].size(); ++n_blocks;
		}
		const size_t used = all ? total : nb * BLOCK_IN;
		bytes_in += (int64_t)used;
		pending.erase(pending.begin(), pending.begin() + used);
		return true;
	}

	bool deflate_block(const uint8_t *src, size_t len, std::vector<uint8_t> &out)
	{
		out.resize(18 + compressBound((uLong)len) + 8 + 64);
		static const uint8_t hdr[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0, 0};
		memcpy(out.data(), hdr, 18);
		for (int lv = level;; lv = 0) { // a block that does not shrink is stored (cannot happen with 65280 input bytes and deflate's 5-byte stored overhead, kept for safety)
			z_stream zs;
			memset(&zs, 0, sizeof zs);
			if (deflateInit2(&zs, lv, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
			zs.next_in = (Bytef *)src; zs.avail_in = (uInt)len;
			zs.next_out = out.data() + 18; zs.avail_out = (uInt)(out.size() - 18 - 8);
			const int rc = deflate(&zs, Z_FINISH);
			const size_t clen = zs.total_out;
			deflateEnd(&zs);
			if (rc != Z_STREAM_END) return false;
			if (18 + clen + 8 <= 65536) {
				w16(out.data() + 16, (uint32_t)(18 + clen + 8 - 1)); // BSIZE = total block size - 1
				w32(out.data() + 18 + clen, (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, (uInt)len));
				w32(out.data() + 18 + clen + 4, (uint32_t)len);
				out.resize(18 + clen + 8);
				return true;
			}
			if (lv == 0) return false;
		}
	}

	bool close()
	{
		bool ok = true;
		if (f) {
			ok = flush(true);
			static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
			if (record_blocks) block_at.push_back(bytes_out);
			if (fwrite(eof, 1, 28, f) != 28) { error = "write failed"; ok = false; }
			if (fclose(f) != 0) { error = "close failed"; ok = false; }
			f = nullptr;
		}
		return ok;
	}
	~BamSink() { if (f) fclose(f); }
};

} // namespace arx

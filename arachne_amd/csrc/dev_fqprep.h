// dev_fqprep.h -- the header standardization (dev_fqstd.h) fused into the sort by barcode (dev_fqsort.h, dev_fqmerge.h): a haplotagging, stLFR or
// TELLseq FASTQ file pair goes in as it is and comes out with the headers `@<id>/1\tBX:Z:<barcode>\tVX:i:<0|1>`, ordered by barcode -- the bytes
// that arx_fastq_sort_ex writes for the files that arx_fastq_standardize writes, without those files.  As the two it is launches over an explicit
// item index, shared by the kernels' driver (hip_fqprep.h) and the host program (tests/fqprepsim/fastq_prepare_sim.cpp) through the same `drv`;
// nothing beyond dev_fqmerge.h's driver is needed (detection, fqs_detect, wants drv.phase as dev_fqstd.h does).
//
// The raw texts stay where they are; there is no standardized copy of them.  The sort's own parse (fs_parse_part: what a record is stays the
// feeder's business) makes the table of the records, FsRec: the four lines of a record in each file.  FpFieldsF, one item per record, adds a
// second row, FpRec: the end of the two header lines (lines 2-4 are what follows, verbatim), id, barcode and v by dev_fqstd.h's rules for
// the one format of the call (fqs_fields), and the sort key.  All positions count from the record's start in R1, so a row is 40 bytes.
//
// The key is what the feeder's rule reads from the COMPOSED R1 header, the value of its leftmost BX:Z:(\S+)\s.  The id stands in front of the
// barcode there and holds no white space, so an id that contains BX:Z: wins: the key is then the id's bytes behind its leftmost BX:Z: followed
// by "/1" (BX:Z: cannot straddle the id and "/1"; "/1" makes the value non-empty, and the '\t' behind it closes it) -- two pieces, the second
// one not in the input.  Otherwise the key is the barcode, which may be empty.  FpKey is the accessor (dev_fqsort.h) that says so: the order
// (fs_order_by), the count of runs and distinct keys, and the key copy of the runs (FxKeepF) all read the key through it, byte by byte.
//
// FpGatherF writes a slab of the output, FS_GATHER_LANES lanes per (sorted record, file): the composed header resolved per output byte from
// the raw R1 text (fqs_header_byte), lines 2-4 copied by bs_copy at the destination's alignment.  Sizes and prefix sums are the composed
// records' (FpKey::size1 / size2).  No byte is written twice, there are no atomics, nothing depends on the order of the items.
//
// Runs (fx_runs_by with FpRows): the run buffers hold raw text; a run's rows are ordered and written to the run files already composed, the
// keys are kept whole ("/1" included), and from there on the merge is dev_fqmerge.h's, unchanged: the run files are standardized text.
//
// Memory per record: the table's 40 bytes (FsRec), this file's 40 (FpRec), two key and two value arrays (24), the two arrays of output
// offsets (16): 120 bytes, against the sort's 80.
#pragma once
#include "dev_fqstd.h"
#include "dev_fqmerge.h"

namespace arx {

enum { FP_W_EXT = FS_W_STAGE1 }; // the merge's stage buffer: the merge starts when the last run's rows are gone
enum { FP_VALID = 1, FP_KEY_IN_ID = 2 };

// what FpFieldsF adds to a record's FsRec.  Positions count from the record's start in R1
struct FpRec { int32_t id_pos, id_len, bc_pos, bc_len, key_pos, key_len /* bytes of the text; "/1" follows with FP_KEY_IN_ID */, h1, h2 /* the header lines, '\n' included */, flags, pad; };

struct FpKey {
	const uint8_t *t1; const FsRec *tab; const FpRec *ext;
	ARX_DEVI int64_t len(int64_t row) const { const FpRec &e = ext[row]; return e.key_len + (e.flags & FP_KEY_IN_ID ? 2 : 0); }
	ARX_DEVI uint8_t byte(int64_t row, int64_t k) const
	{
		const FpRec &e = ext[row];
		return k < e.key_len ? t1[tab[row].off1 + e.key_pos + k] : k == e.key_len ? (uint8_t)'/' : (uint8_t)'1';
	}
	ARX_DEVI int64_t size1(int64_t row) const { const FpRec &e = ext[row]; return (int64_t)FQS_FIXED + e.id_len + e.bc_len + (tab[row].len1 - e.h1); }
	ARX_DEVI int64_t size2(int64_t row) const { const FpRec &e = ext[row]; return (int64_t)FQS_FIXED + e.id_len + e.bc_len + (tab[row].len2 - e.h2); }
};

struct FpFieldsF { // item: one record of the table, for the format of the call.  cnt: has a barcode | is valid << 32
	const uint8_t *t1, *t2; const FsRec *tab; int32_t format; FpRec *ext; int64_t *cnt;
	ARX_DEVI void operator()(int64_t r) const
	{
		const FsRec &rec = tab[r];
		const uint8_t *t = t1 + rec.off1, *u = t2 + rec.off2;
		FpRec e;
		// a record is four whole lines in each file: its first newline ends the header
		e.h1 = 0;
		while (e.h1 < rec.len1 && t[e.h1] != '\n') ++e.h1;
		e.h1 += e.h1 < rec.len1;
		e.h2 = 0;
		while (e.h2 < rec.len2 && u[e.h2] != '\n') ++e.h2;
		e.h2 += e.h2 < rec.len2;
		FqsRec o;
		const bool have = fqs_fields(t, 1, e.h1, format, o);
		e.id_pos = o.id_pos; e.id_len = o.id_len; e.bc_pos = o.bc_pos; e.bc_len = o.bc_len;
		e.flags = o.v ? FP_VALID : 0; e.pad = 0;
		e.key_pos = o.bc_pos; e.key_len = o.bc_len;
		const int32_t id_end = o.id_pos + o.id_len;
		for (int32_t p = o.id_pos; p + 5 <= id_end; ++p)
			if (fqs_tag(t, p, id_end, 'B', 'X', 'Z')) { e.key_pos = p + 5; e.key_len = id_end - (p + 5); e.flags |= FP_KEY_IN_ID; break; }
		ext[r] = e;
		cnt[r] = (int64_t)have | (int64_t)(o.v != 0) << 32;
	}
};

struct FpGatherF { // item: one lane of one file of one sorted record of the slab that starts at sorted record j0
	FsText t; FpKey key; const uint32_t *vals; const int64_t *out1, *out2; int64_t j0; uint8_t *d1, *d2;
	ARX_DEVI void operator()(int64_t i) const
	{
		const int lane = (int)(i % FS_GATHER_LANES);
		const bool two = (i / FS_GATHER_LANES) & 1;
		const int64_t j = j0 + i / (2 * FS_GATHER_LANES), row = vals[j];
		const FsRec &r = key.tab[row];
		const FpRec &e = key.ext[row];
		const FqsRec q = {e.id_pos, e.id_len, e.bc_pos, e.bc_len, 0, 0, 0, 0, e.flags & FP_VALID, 0};
		uint8_t *d = two ? d2 + (out2[j] - out2[j0]) : d1 + (out1[j] - out1[j0]);
		const int32_t h = FQS_FIXED + e.id_len + e.bc_len;
		for (int32_t k = lane; k < h; k += FS_GATHER_LANES) d[k] = fqs_header_byte(t.t1 + r.off1, q, two, k);
		if (two) bs_copy(d + h, t.t2 + r.off2 + e.h2, r.len2 - e.h2, lane, FS_GATHER_LANES);
		else bs_copy(d + h, t.t1 + r.off1 + e.h1, r.len1 - e.h1, lane, FS_GATHER_LANES);
	}
};

// the records of a prepared sort (dev_fqmerge.h: FxPlainRows): fields and key per record of the table, the composing gather, a key for the host
struct FpRows {
	int32_t format = FQS_UNKNOWN;
	int64_t with_bc = 0, valid = 0; // over every table that key() has seen
	template <class Drv> FpKey key(Drv &drv, const FsText &T, const FsRec *tab, int64_t n, FsSortMem &m)
	{
		if (n <= 0) return FpKey{T.t1, tab, nullptr};
		FpRec *ext = (FpRec *)drv.work(FP_W_EXT, (int64_t)sizeof(FpRec) * n);
		int64_t *cnt = (int64_t *)m.keys[0]; // the order has not begun: its arrays are free
		drv.items("fp_fields", n, FpFieldsF{T.t1, T.t2, tab, format, ext, cnt});
		drv.scan(cnt, m.out1, n);
		const int64_t both = drv.get(&m.out1[n]);
		with_bc += both & 0xffffffff; valid += both >> 32;
		return FpKey{T.t1, tab, ext};
	}
	template <class Drv, class Sink> void gather(Drv &drv, const FsText &T, const FpKey &key, int64_t n, const FsSortMem &m, int64_t slab, int64_t longest, Sink &sink, FsCounts &c)
	{
		fs_gather_by(drv, n, m, slab, longest, sink, c, "fp_gather",
		             [&](int64_t j0, uint8_t *d1, uint8_t *d2) { return FpGatherF{T, key, m.vals[m.cur], m.out1, m.out2, j0, d1, d2}; });
	}
	template <class Drv> std::vector<uint8_t> key_bytes(Drv &drv, const FpKey &key, int64_t row)
	{
		FsRec r;
		FpRec e;
		drv.fetch(&r, key.tab + row, sizeof r);
		drv.fetch(&e, key.ext + row, sizeof e);
		std::vector<uint8_t> b((size_t)e.key_len);
		if (e.key_len) drv.fetch(b.data(), key.t1 + r.off1 + e.key_pos, (size_t)e.key_len);
		if (e.flags & FP_KEY_IN_ID) { b.push_back('/'); b.push_back('1'); }
		return b;
	}
};

// the table of two whole texts (drv.table(), N records: fs_parse made it) ordered by the composed key -> the longest composed record
template <class Drv> int64_t fp_order(Drv &drv, const FsText &T, int64_t N, FpRows &rows, FsSortMem &m, FsCounts &c, FpKey &key)
{
	const FsRec *tab = N ? drv.table(N) : nullptr;
	fs_sort_mem(drv, N, m);
	key = rows.key(drv, T, tab, N, m);
	return fs_order_by(drv, key, N, m, c);
}

} // namespace arx

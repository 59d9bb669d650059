// dev_fqsort.h -- the sort of a FASTQ file pair by barcode (the reference's `preprocess`: samtools import | sort -t BX | fastq) as launches over
// an explicit item index: the table of the records, their order, the gather of the sorted records.  hip_fqsort.h runs the functors below as
// kernels, one item per thread, the key sort through rocprim; tests/fqsortsim/fastq_sort_sim.cpp runs the very same functions on the host, the
// items of a launch in a loop, in either order.  Nothing here knows which of the two it is: a driver `drv` supplies
//     drv.items(name, n, f)                          f(i) for every i in [0, n), in any order, all done when the next call starts
//     drv.scan(in, out, n) / drv.scan32(in, out, n)  out[0..n]: the exclusive prefix sums of in[0..n), out[n] the total (scan32 returns it)
//     drv.max64(in, n) / drv.or64(in, n)             the maximum / the bitwise OR of n unsigned 64-bit words (0 for none)
//     drv.get(p) / drv.fetch(host, dev, bytes)       the launches' memory read by the host
//     drv.sort_pairs(kin, kout, vin, vout, n, bits)  a STABLE sort of n (key, value) pairs by the low `bits` bits of the key
//     drv.work(slot, bytes)                          the work buffer `slot` with room for `bytes` (16-byte aligned; what it held is gone)
//     drv.table(n)                                   the record table with room for n records; the records it holds stay
//
// What a record and its barcode are is the feeder's business (dev_fastq.h, feeder.h): the table is made by the feeder's own functors -- line
// index (KNlCount, KNlFill), state scan (KLineMaps, KLineStates, KRecCount, KRecFill) and KRecParse with its BX:Z: rule -- window by window
// over the two texts, which stay where they are in device memory.  Those functors want a 16-byte-aligned window and count in int32, so a
// window is copied to an aligned buffer first (FsWindowF: the feeder moves its carry the same way); a parse consumes the line pairs both
// windows hold, up to the last record that is whole in both, and the next window starts at the first line that was not consumed, so every
// parse starts in the search state.  A line or a record that a full window does not hold is FS_E_TOO_LARGE.  The four lines of a record
// follow one another in their file, so per record and file ONE range [off, off + len) is the four lines verbatim, newlines included.
//
// Order.  Barcodes are byte strings of any length; the order is byte-wise, unsigned, a proper prefix first, equal barcodes in input order.
// That is the order of the tuple (chunk 0, chunk 1, ..., chunk C - 1, length), chunk c being bytes [8c, 8c + 8) big-endian and zero-padded:
// a least-significant-digit chain of stable sorts, the length first, then the chunks from the last to the first, each chunk gathered through
// the permutation so far.  The length pass is what tells AB from AB\0.  C = ceil(longest barcode / 8), by a reduction; a pass sorts only the
// bits in which its keys differ (the OR over key ^ first key, by a reduction too) and is left out where they do not differ at all.  The
// passes read a key through an accessor (fs_order_by; FsPlainKey: the barcode where it lies in R1's text), so that a key need not be one
// substring of the input (dev_fqprep.h).
//
// Output.  The sorted sizes' prefix sums per file say where every record goes.  The output is made in slabs: a range of sorted records
// whose bytes fit slab_bytes in both files, at least one record; FS_GATHER_LANES lanes copy one record of one file (bs_copy: the two
// alignments are independent).  A sink takes the slabs: sink.take(k, cap, b1, b2, &d1, &d2) hands out the two buffers of slab k (b1 and b2 bytes will be
// written; no slab takes more than cap), sink.give(k, j0, j1, b1, b2) is told that the gather of sorted records [j0, j1) into them has been started.
//
// Memory per record: the table's 40 bytes (FsRec), two key and two value arrays (24), the two arrays of output offsets (16): 80 bytes.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "arx_hd.h"
#include "dev_fastq.h"
#include "dev_bamsort.h"

namespace arx {

constexpr int64_t FS_MIN_WINDOW = 128;               // window_bytes below this are refused: every line and record must fit a window
constexpr int64_t FS_MAX_WINDOW = (int64_t)1 << 29;  // dev_fastq.h counts in int32, and the two windows share one line index
constexpr int FS_GATHER_LANES = 16;                  // lanes that copy one record of one file
enum { FS_OK = 0, FS_E_TOO_LARGE = 1, FS_E_RECORDS = 2 };
enum { FS_W_WIN1 = 0, FS_W_WIN2, FS_W_CNT, FS_W_OFF, FS_W_NL, FS_W_BMAP, FS_W_BSTATE, FS_W_HDR, FS_W_RCNT, FS_W_ROFF, FS_W_RECL, FS_W_TMP, FS_W_SC, FS_W_VALID, FS_W_META,
       FS_W_KEYS0, FS_W_KEYS1, FS_W_VALS0, FS_W_VALS1, FS_W_OUT1, FS_W_OUT2,
       FS_W_KOFF, FS_W_FIRST, FS_W_RANGE, FS_W_DELTA, FS_W_STAGE1, FS_W_STAGE2, // dev_fqmerge.h
       FS_N_WORK };

struct FsRec { int64_t off1, off2, bc_off; int32_t len1, len2, bc_len, pad; }; // the record's lines in R1 and R2, its barcode in R1's text
// the table grows by half: what a driver allocates when n records are asked for and the table holds fewer
ARX_HDI int64_t fs_table_room(int64_t n) { return n + n / 2; }
struct FsText { const uint8_t *t1, *t2; int64_t n1, n2; };
struct FsCounts { int64_t n_records, skipped, runs_in, distinct, max_bc, passes, windows, slabs, bytes1, bytes2; };

// a feeder functor (item, slot) under an int64 item index
template <class K> struct FsWide {
	K k;
	ARX_DEVI void operator()(int64_t i) const { k((int)i, 0); }
};
template <class K> ARX_HDI FsWide<K> fs_wide(const K &k) { return FsWide<K>{k}; }

// ---- the window: src[0, n) to the aligned dst, 16 bytes per item; what the last word holds past n is zero
struct FsWindowF {
	const uint8_t *src; int64_t n; uint8_t *dst;
	ARX_DEVI void operator()(int64_t i) const
	{
		const int64_t b = 16 * i, left = n - b;
		uint8_t *d = (uint8_t *)__builtin_assume_aligned(dst + b, 16);
		if (left >= 16) { FqWord16 v; memcpy(&v, src + b, 16); *(FqWord16 *)d = v; return; }
		for (int k = 0; k < 16; ++k) d[k] = k < left ? src[b + k] : (uint8_t)0;
	}
};
// what KRecParse found of record r of a window whose texts start at a1 and a2 of the files -> the table
struct FsStoreF {
	FqLines ln; const int32_t *rec_line; const FqRecTmp *tmp; int64_t a1, a2; FsRec *out;
	ARX_DEVI void operator()(int64_t r) const
	{
		const int j = rec_line[r];
		const int32_t s1 = ln.start1(j), s2 = ln.start2(j);
		FsRec o;
		o.off1 = a1 + s1; o.len1 = ln.nl1[j + 3] + 1 - s1;
		o.off2 = a2 + s2; o.len2 = ln.nl2[j + 3] + 1 - s2;
		o.bc_off = a1 + tmp[r].bc_pos; o.bc_len = tmp[r].bc_len; o.pad = 0;
		out[r] = o;
	}
};

// ---- the order.  What is ordered is seen through a key accessor K (rows are numbered as the table's):
//     K.len(row)       the key's length             K.byte(row, k)   its byte k, 0 <= k < len
//     K.size1(row) / K.size2(row)                   the bytes the row's record takes in the two outputs
// FsPlainKey is arx_fastq_sort's: the barcode where the parse found it in R1's text, the record's lines verbatim.  dev_fqprep.h has a key in
// two pieces and records whose header is composed
ARX_HDI int fs_bits(uint64_t x) { int b = 0; while (b < 64 && (x >> b) != 0) ++b; return b; }
struct FsPlainKey {
	const uint8_t *t1; const FsRec *tab;
	ARX_DEVI int64_t len(int64_t row) const { return tab[row].bc_len; }
	ARX_DEVI uint8_t byte(int64_t row, int64_t k) const { return t1[tab[row].bc_off + k]; }
	ARX_DEVI int64_t size1(int64_t row) const { return tab[row].len1; }
	ARX_DEVI int64_t size2(int64_t row) const { return tab[row].len2; }
};
// chunk c of a key: bytes [8c, 8c + 8), the first one on top, zeros behind the key's end
template <class K> ARX_DEVI uint64_t fs_chunk(const K &key, int64_t row, int64_t c)
{
	uint64_t k = 0;
	const int64_t n = key.len(row);
	for (int64_t x = 8 * c; x < 8 * c + 8; ++x) k = k << 8 | (x < n ? key.byte(row, x) : 0u);
	return k;
}
template <class K> struct FsLenKeyF { // the least significant key: the length; the permutation starts as the identity
	K key; uint64_t *keys, *diff; uint32_t *vals;
	ARX_DEVI void operator()(int64_t j) const
	{
		const uint64_t k = (uint64_t)(uint32_t)key.len(j);
		keys[j] = k; diff[j] = k ^ (uint64_t)(uint32_t)key.len(0); vals[j] = (uint32_t)j;
	}
};
template <class K> struct FsChunkKeyF { // keys[j]: chunk c of the record at place j of the permutation so far; diff[j]: the bits in which it differs from place 0's
	K key; const uint32_t *vals; int64_t c; uint64_t *keys, *diff;
	ARX_DEVI void operator()(int64_t j) const
	{
		const uint64_t k = fs_chunk(key, vals[j], c);
		keys[j] = k; diff[j] = k ^ fs_chunk(key, vals[0], c);
	}
};
// KRunFlag's rule (dev_fastq.h) on the table: place j opens a run iff its key (bytes and length) differs from place j - 1's.  vals: the
// order the places are taken in; null: the input's
template <class K> struct FsRunF {
	K key; const uint32_t *vals; int64_t *flag;
	ARX_DEVI void operator()(int64_t j) const
	{
		bool open = true;
		if (j > 0) {
			const int64_t a = vals ? (int64_t)vals[j] : j, q = vals ? (int64_t)vals[j - 1] : j - 1, n = key.len(a);
			open = key.len(q) != n;
			for (int64_t k = 0; !open && k < n; ++k) open = key.byte(q, k) != key.byte(a, k);
		}
		flag[j] = open;
	}
};

// ---- gather
template <class K> struct FsSizesF {
	K key; const uint32_t *vals; int64_t *s1, *s2;
	ARX_DEVI void operator()(int64_t j) const { s1[j] = key.size1(vals[j]); s2[j] = key.size2(vals[j]); }
};
struct FsGatherF { // item: one lane of one file of one sorted record of the slab that starts at sorted record j0
	FsText t; const FsRec *tab; const uint32_t *vals; const int64_t *out1, *out2; int64_t j0; uint8_t *d1, *d2;
	ARX_DEVI void operator()(int64_t i) const
	{
		const int lane = (int)(i % FS_GATHER_LANES);
		const bool two = (i / FS_GATHER_LANES) & 1;
		const int64_t j = j0 + i / (2 * FS_GATHER_LANES);
		const FsRec &r = tab[vals[j]];
		if (two) bs_copy(d2 + (out2[j] - out2[j0]), t.t2 + r.off2, r.len2, lane, FS_GATHER_LANES);
		else bs_copy(d1 + (out1[j] - out1[j0]), t.t1 + r.off1, r.len1, lane, FS_GATHER_LANES);
	}
};

// ---- the table: every record of the two texts, in input order.  FS_OK: c.n_records, c.skipped, c.windows are set and drv.table() holds the
// records; FS_E_TOO_LARGE: a line or a record does not fit a window of `window` bytes; FS_E_RECORDS: more than 2^32 - 1 records.
// fs_parse_part is the parse of a text that may be a part of its file (dev_fqmerge.h: a run).  open1 / open2: the file goes on behind T.n1 /
// T.n2, so the text's end is no end of input: the parse stops behind the first window that touches such an end, ended = false, and
// [a1, T.n1), [a2, T.n2) are the line pairs it did not consume -- they start in the search state, as every window does -- for the caller to
// put in front of what follows; lines: the line pairs consumed.  The end-of-input rule is applied only where a closed end is reached
struct FsPart { bool open1 = false, open2 = false; int64_t n_before = 0; /* records of earlier parts */ int64_t a1 = 0, a2 = 0, lines = 0; bool ended = true; };
template <class Drv> int fs_parse_part(Drv &drv, const FsText &T, int64_t window, FsCounts &c, FsPart &p)
{
	int64_t a1 = 0, a2 = 0, N = 0;
	p.a1 = p.a2 = p.lines = 0; p.ended = true;
	c.n_records = c.skipped = c.windows = 0;
	for (;;) {
		const int64_t w1 = T.n1 - a1 < window ? T.n1 - a1 : window, w2 = T.n2 - a2 < window ? T.n2 - a2 : window;
		const bool at1 = a1 + w1 == T.n1, at2 = a2 + w2 == T.n2, end1 = at1 && !p.open1, end2 = at2 && !p.open2;
		const int32_t nw1 = (int32_t)((w1 + 15) / 16), nw2 = (int32_t)((w2 + 15) / 16), nw = nw1 + nw2;
		++c.windows;
		int32_t L1 = 0, L2 = 0;
		FqWin w{nullptr, nullptr, (int32_t)w1, (int32_t)w2, nw1, nw2};
		const int32_t *nl = nullptr;
		if (nw > 0) {
			uint8_t *b1 = (uint8_t *)drv.work(FS_W_WIN1, 16 * (int64_t)nw1), *b2 = (uint8_t *)drv.work(FS_W_WIN2, 16 * (int64_t)nw2);
			drv.items("fs_window", nw1, FsWindowF{T.t1 + a1, w1, b1});
			drv.items("fs_window", nw2, FsWindowF{T.t2 + a2, w2, b2});
			w.t1 = b1; w.t2 = b2;
			int32_t *cnt = (int32_t *)drv.work(FS_W_CNT, 4 * (int64_t)nw), *off = (int32_t *)drv.work(FS_W_OFF, 4 * ((int64_t)nw + 1));
			drv.items("fq_nl_count", nw, fs_wide(KNlCount{w, cnt}));
			const int64_t total = drv.scan32(cnt, off, nw);
			L1 = drv.get32(off + nw1);
			L2 = (int32_t)(total - L1);
			int32_t *nlw = (int32_t *)drv.work(FS_W_NL, 4 * total);
			drv.items("fq_nl_fill", nw, fs_wide(KNlFill{w, off, nlw}));
			nl = nlw;
		}
		const int32_t L = L1 < L2 ? L1 : L2;
		int32_t meta[3] = {0, 0, 0};
		int64_t n = 0;
		if (L > 0) {
			const FqLines ln{w.t1, w.t2, nl, nl + L1, L};
			const int nblk = (L + FQ_LINE_BLOCK - 1) / FQ_LINE_BLOCK;
			uint8_t *bmap = (uint8_t *)drv.work(FS_W_BMAP, nblk), *bstate = (uint8_t *)drv.work(FS_W_BSTATE, nblk), *hdr = (uint8_t *)drv.work(FS_W_HDR, L);
			int32_t *rcnt = (int32_t *)drv.work(FS_W_RCNT, 4 * (int64_t)nblk), *roff = (int32_t *)drv.work(FS_W_ROFF, 4 * ((int64_t)nblk + 1));
			int32_t *dmeta = (int32_t *)drv.work(FS_W_META, 4 * 3);
			drv.items("fq_line_maps", nblk, fs_wide(KLineMaps{ln, bmap, hdr}));
			drv.items("fq_line_states", 1, fs_wide(KLineStates{ln, bmap, bstate, nblk, 0, dmeta}));
			drv.items("fq_rec_count", nblk, fs_wide(KRecCount{ln, bstate, hdr, rcnt, dmeta}));
			n = drv.scan32(rcnt, roff, nblk);
			if (p.n_before + N + n > (int64_t)UINT32_MAX) return FS_E_RECORDS;
			if (n > 0) {
				const int32_t ni = (int32_t)n;
				int32_t *recl = (int32_t *)drv.work(FS_W_RECL, 4 * n), *sc = (int32_t *)drv.work(FS_W_SC, 16 * n);
				FqRecTmp *tmp = (FqRecTmp *)drv.work(FS_W_TMP, (int64_t)sizeof(FqRecTmp) * n);
				uint8_t *valid = (uint8_t *)drv.work(FS_W_VALID, n);
				FsRec *tab = drv.table(N + n);
				drv.items("fq_rec_fill", nblk, fs_wide(KRecFill{ln, bstate, hdr, roff, recl}));
				drv.items("fq_rec_parse", n, fs_wide(KRecParse{ln, recl, ni, tmp, sc, valid}));
				drv.items("fs_store", n, FsStoreF{ln, recl, tmp, a1, a2, tab + N});
			}
			drv.fetch(meta, dmeta, sizeof meta);
		}
		c.skipped += meta[2] - 4 * n; // every consumed line is a skipped one or belongs to one of the n records
		N += n;
		// a file that is at its end and has no line left ends the input: an unterminated last line does not count, nor what the other
		// file still has, and the record the end cut off does not exist
		if ((end1 && L1 == L) || (end2 && L2 == L)) break;
		a1 += meta[0]; a2 += meta[1];
		p.lines += meta[2];
		if ((at1 && p.open1) || (at2 && p.open2)) { p.a1 = a1; p.a2 = a2; p.ended = false; break; }
		if (meta[2] == 0) return FS_E_TOO_LARGE; // a full window, and not one line pair of it could be consumed
	}
	c.n_records = N;
	return FS_OK;
}
template <class Drv> int fs_parse(Drv &drv, const FsText &T, int64_t window, FsCounts &c)
{
	FsPart whole;
	return fs_parse_part(drv, T, window, c, whole);
}

struct FsSortMem { uint64_t *keys[2]; uint32_t *vals[2]; int64_t *out1, *out2; int cur; }; // vals[cur]: the order
template <class Drv> void fs_sort_mem(Drv &drv, int64_t N, FsSortMem &m)
{
	m.keys[0] = (uint64_t *)drv.work(FS_W_KEYS0, 8 * N); m.keys[1] = (uint64_t *)drv.work(FS_W_KEYS1, 8 * N);
	m.vals[0] = (uint32_t *)drv.work(FS_W_VALS0, 4 * N); m.vals[1] = (uint32_t *)drv.work(FS_W_VALS1, 4 * N);
	m.out1 = (int64_t *)drv.work(FS_W_OUT1, 8 * (N + 1)); m.out2 = (int64_t *)drv.work(FS_W_OUT2, 8 * (N + 1));
	m.cur = 0;
}
template <class Drv, class K> int64_t fs_count_runs(Drv &drv, const K &key, const uint32_t *vals, int64_t N, FsSortMem &m)
{
	drv.items("fs_run", N, FsRunF<K>{key, vals, (int64_t *)m.keys[0]});
	drv.scan((const int64_t *)m.keys[0], m.out1, N);
	return drv.get(&m.out1[N]);
}
// the runs of the input, the order (m.vals[m.cur]), the distinct keys, and m.out1 / m.out2[0 .. N]: where the sorted records start in
// the two outputs.  -> the longest record of either file
template <class Drv, class K> int64_t fs_order_by(Drv &drv, const K &key, int64_t N, FsSortMem &m, FsCounts &c)
{
	c.runs_in = c.distinct = c.max_bc = c.passes = c.bytes1 = c.bytes2 = 0;
	if (N == 0) return 0;
	c.runs_in = fs_count_runs(drv, key, nullptr, N, m);
	drv.items("fs_len_key", N, FsLenKeyF<K>{key, m.keys[0], m.keys[1], m.vals[0]});
	c.max_bc = (int64_t)drv.max64(m.keys[0], N);
	m.cur = 0;
	if (const uint64_t differ = drv.or64(m.keys[1], N)) {
		drv.sort_pairs(m.keys[0], m.keys[1], m.vals[0], m.vals[1], N, fs_bits(differ));
		m.cur = 1; ++c.passes;
	}
	for (int64_t ch = (c.max_bc + 7) / 8 - 1; ch >= 0; --ch) {
		drv.items("fs_chunk_key", N, FsChunkKeyF<K>{key, m.vals[m.cur], ch, m.keys[0], m.keys[1]});
		const uint64_t differ = drv.or64(m.keys[1], N);
		if (!differ) continue;
		drv.sort_pairs(m.keys[0], m.keys[1], m.vals[m.cur], m.vals[m.cur ^ 1], N, fs_bits(differ));
		m.cur ^= 1; ++c.passes;
	}
	c.distinct = fs_count_runs(drv, key, m.vals[m.cur], N, m);
	drv.items("fs_sizes", N, FsSizesF<K>{key, m.vals[m.cur], (int64_t *)m.keys[0], (int64_t *)m.keys[1]});
	const uint64_t big1 = drv.max64(m.keys[0], N), big2 = drv.max64(m.keys[1], N);
	drv.scan((const int64_t *)m.keys[0], m.out1, N);
	drv.scan((const int64_t *)m.keys[1], m.out2, N);
	c.bytes1 = drv.get(&m.out1[N]); c.bytes2 = drv.get(&m.out2[N]);
	return (int64_t)(big1 > big2 ? big1 : big2);
}
template <class Drv> int64_t fs_order(Drv &drv, const FsText &T, const FsRec *tab, int64_t N, FsSortMem &m, FsCounts &c)
{
	return fs_order_by(drv, FsPlainKey{T.t1, tab}, N, m, c);
}
// the sorted records to the sink, slab by slab; make(j0, d1, d2): the functor that writes the slab that starts at sorted record j0, started
// under `name` with FS_GATHER_LANES items per record and file
template <class Drv, class Sink, class Make> void fs_gather_by(Drv &drv, int64_t N, const FsSortMem &m, int64_t slab_bytes, int64_t longest, Sink &sink, FsCounts &c, const char *name, Make make)
{
	const int64_t cap = slab_bytes > longest ? slab_bytes : longest;
	c.slabs = 0;
	int64_t at1 = 0, at2 = 0; // out1[j0], out2[j0]
	for (int64_t j0 = 0; j0 < N;) {
		// the last j1 in (j0, N] at which both files' bytes still fit slab_bytes, or j0 + 1: one record always goes, the buffers hold the longest
		int64_t lo = j0 + 1, hi = N, e1 = 0, e2 = 0;
		while (lo < hi) {
			const int64_t mid = lo + (hi - lo + 1) / 2;
			if (drv.get(&m.out1[mid]) - at1 <= slab_bytes && drv.get(&m.out2[mid]) - at2 <= slab_bytes) lo = mid; else hi = mid - 1;
		}
		e1 = drv.get(&m.out1[lo]); e2 = drv.get(&m.out2[lo]);
		uint8_t *d1 = nullptr, *d2 = nullptr;
		sink.take(c.slabs, cap, e1 - at1, e2 - at2, &d1, &d2);
		drv.items(name, (lo - j0) * 2 * FS_GATHER_LANES, make(j0, d1, d2));
		sink.give(c.slabs, j0, lo, e1 - at1, e2 - at2);
		++c.slabs;
		j0 = lo; at1 = e1; at2 = e2;
	}
}
template <class Drv, class Sink> void fs_gather(Drv &drv, const FsText &T, const FsRec *tab, int64_t N, const FsSortMem &m, int64_t slab_bytes, int64_t longest, Sink &sink, FsCounts &c)
{
	fs_gather_by(drv, N, m, slab_bytes, longest, sink, c, "fs_gather",
	             [&](int64_t j0, uint8_t *d1, uint8_t *d2) { return FsGatherF{T, tab, m.vals[m.cur], m.out1, m.out2, j0, d1, d2}; });
}

} // namespace arx

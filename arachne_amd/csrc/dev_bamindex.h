// dev_bamindex.h -- the BAI index of one coordinate-sorted BAM record stream (the SAM specification, 5.2 and 5.3; include/arachne_amd.h states the
// contract in full), as launches over an explicit item index in the manner of dev_bamsort.h, whose record discovery it uses unchanged.
// hip_bamindex.h runs the functors below as kernels, one item per thread; tests/baisim/bam_index_sim.cpp runs the very same functions on the
// host, the items of a launch in a loop, in either order.  Beside dev_bamsort.h's items / scan / get / put / sort_pairs a driver supplies
//     Drv::Buf                          memory of the launches with a scope: alloc(bytes), release(), as<T>(), p
//     drv.upload(d, h, n) / drv.fetch(h, d, n) / drv.copy(d, d2, n) / drv.fill(d, byte, n)     all done when they return
//     drv.scan(in, out, n, name)        the name says which phase the time is booked under
// and a source `src` the bytes: src.load(k, dst, n) puts the n inflated bytes of slab k at dst (false: a block does not inflate).
//
// The stream is indexed slab by slab (a slab: a run of whole BGZF blocks, BiBlocks::cut).  The buffer of a slab holds the stream's bytes
// [g0, b): in front of the slab's own bytes [a, b) lies what the slab before could not finish -- the record whose fixed 36 bytes, name and
// CIGAR were not whole in it (at most the last one found), or a cut block_size field.  The chain enters the buffer where it left the last,
// so a record is met exactly once, and one larger than a slab simply grows in the carry until its CIGAR is whole.  The rows of the blocks the
// buffer's bytes lie in are uploaded with it (the host holds the whole table), so V(start) is a binary search over the buffer's own rows.
//   per record    bi_rec: V(start); the rules on refID, pos and end; end from the CIGAR; bin = the scheme's bin of [beg, end); the (mapped, unmapped) count
//                 word; the linear index by a 64-bit atomic minimum of V(start) over the record's windows, which no order can change
//                 bi_flag: the order check against the predecessor and the run-start flag (the slab's first record against the carried last)
//                 Offences go into one error word by an atomic minimum of (record number << 8 | rule): the first offending record wins
//   runs          scans of the flags and of the count words; bi_runs compacts (refID << bin_bits | bin, V(begin), V(end), counts) at the run starts.
//                 A run ends where the next begins; the slab's last run ends at V(the next chain offset), which the host knows
//   chunks        a stable sort of the runs by (refID, bin); bi_head marks where a sorted run cannot join its predecessor (another bin, or
//                 (earlier.end >> 16) < (later.beg >> 16)); a scan; bi_chunks compacts the joined chunks, which the host fetches and appends
//                 bin by bin under the same rule (bi_append).  The rule relates two neighbours only and a run cut by a slab border ends where
//                 its rest begins, so the chunks do not depend on where the slabs were cut
// Records with refID = -1 form a run under refID = n_ref, which the host drops; their number is what the count words leave of the records.
// The bins and the windows follow a scheme (BiScheme: min_shift, depth) that the functors carry as a value.  The BAI is (14, 5); under the
// scheme of a CSI index (bi_csi_scheme) the same run serves contigs of up to 2^31 - 1 bases, the window table is what the bins' loffset is
// read from (bi_serialise_csi), and the run key refID << bin_bits | bin widens with the depth.
// Nothing here depends on the order of the items: every write goes to a slot of its own item, or is a minimum or a sum.
// The slab body is stated once (BiSlabs) and driven from two sides: bi_run pulls the slabs of a finished file from `src`; BiPush is handed the
// record stream by a writer while it appends, feed by feed, with the closed form P in place of V until the writer's block table is known
// (tests/bixsim/bam_index_feeds_sim.cpp runs that side on the host).
#pragma once
#include <stdint.h>
#include <string.h>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include "dev_bamsort.h"

namespace arx {

constexpr int BI_LIN_SHIFT = 14;                       // a window of the BAI's linear index: 16384 bases
constexpr uint32_t BI_PSEUDO_BIN = 37450;
constexpr int BI_CSI_SHIFT_MIN = 10, BI_CSI_SHIFT_MAX = 24, BI_CSI_SHIFT_DEFAULT = 14;
constexpr int64_t BI_MAX_REF = (int64_t)1 << 29;       // the BAI format's limit
constexpr int64_t BI_MAX_AT = (int64_t)1 << 48;        // a virtual offset holds 48 bits of file offset
constexpr uint64_t BI_UNSET = ~(uint64_t)0;
enum { BI_OK = 0, BI_E_CHAIN = 1, BI_E_INFLATE = 2, BI_E_RULE = 3 };
enum { BI_R_FIELDS = 1, BI_R_REFID, BI_R_POS, BI_R_END, BI_R_ORDER };
enum { BI_W_ERR = 0, BI_W_NP, BI_W_FROM, BI_W_CONT, BI_W_LASTKEY, BI_W_LASTRB, BI_W_RUNS, BI_N_WORDS };

// The bin scheme, a value the functors carry: levels 0 .. depth, a bin of level l spans 2^(min_shift + 3 (depth - l)) bases, the windows of the
// offset table 2^min_shift (the leaf bins' width).  The BAI (the SAM specification, 5.3) is the instance (14, 5); a CSI index (CSIv1) states its
// own.  depth <= 7 (min_shift >= 10 and 2^31 - 1 bases at most), so a bin number is below 2^22 and fits the 3 depth + 1 bits of the run key
struct BiScheme {
	int32_t min_shift, depth;
	ARX_HDI int bin_bits() const { return 3 * depth + 1; }                                     // (8^(depth+1) - 1) / 7 < 2^(3 depth + 1)
	ARX_HDI uint32_t first(int l) const { return (uint32_t)((((uint64_t)1 << (3 * l)) - 1) / 7); } // the first bin of level l
	ARX_HDI uint32_t meta() const { return first(depth + 1) + 1; }                             // the pseudo-bin: 37450 at depth 5
	// the bin of the zero-based half-open interval [beg, end): the deepest level at which beg and end - 1 lie in one bin
	ARX_HDI uint32_t bin(int64_t beg, int64_t end) const
	{
		--end;
		int s = min_shift;
		for (int l = depth; l > 0; --l, s += 3)
			if (beg >> s == end >> s) return first(l) + (uint32_t)(beg >> s);
		return 0;
	}
	// the first window of a bin's interval
	ARX_HDI int64_t first_window(uint32_t b) const
	{
		int l = depth;
		while (first(l) > b) --l;
		return (int64_t)(b - first(l)) << (3 * (depth - l));
	}
};
constexpr BiScheme BI_BAI = {BI_LIN_SHIFT, 5};
ARX_HDI uint32_t bi_reg2bin(int64_t beg, int64_t end) { return BI_BAI.bin(beg, end); } // the SAM specification, 5.3

// the non-empty blocks a buffer's bytes lie in: ooff[i] is where block i's bytes start in the buffer (the first may start in front of it), at[i]
// its file offset
struct BiRows { const int64_t *ooff, *at; int64_t n; };
// V(o) for an offset o of the buffer that lies in one of the n >= 1 rows
ARX_HDI uint64_t bi_voff(const BiRows &r, int64_t o)
{
	int64_t lo = 0, hi = r.n; // the last row that starts at or before o
	while (hi - lo > 1) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (r.ooff[mid] <= o) lo = mid; else hi = mid;
	}
	return (uint64_t)r.at[lo] << 16 | (uint64_t)(o - r.ooff[lo]);
}
// The second source of offsets, a closed form: a writer (bam_sink.h) lays its stream out before any compressed size is known -- the header ends
// its own hb = ceil(H / BI_BLOCK) blocks, every block behind it but the last holds BI_BLOCK bytes -- so the byte r of the record stream lies in block
// hb + r / BI_BLOCK at r % BI_BLOCK.  P(r) = block ordinal << 16 | offset within stands in for V until the writer has closed: file offsets grow
// strictly with the ordinal, so P orders as V does, the join rule decides the same, and the windows' minima pick the same records.  BiPush::finish
// turns P into V by one lookup in the table of block offsets
constexpr int64_t BI_BLOCK = 0xff00; // BamSink::BLOCK_IN
ARX_HDI int64_t bi_header_blocks(int64_t H) { return (H + BI_BLOCK - 1) / BI_BLOCK; }
ARX_HDI uint64_t bi_poff(int64_t hb, int64_t r) { return (uint64_t)(hb + r / BI_BLOCK) << 16 | (uint64_t)(r % BI_BLOCK); }
// where a buffer's bytes lie: rows.n > 0 -- in the rows of a file; else by the closed form, byte 0 of the buffer being byte `base` of the record stream
struct BiOff { BiRows rows; int64_t base, hb; };
ARX_HDI uint64_t bi_off(const BiOff &f, int64_t o) { return f.rows.n > 0 ? bi_voff(f.rows, o) : bi_poff(f.hb, f.base + o); }
// P -> V, one item per window of the table; an unset window stays unset.  p_total: P(the stream's size), which no start equals -- the contract's
// V(total) is the EOF block's offset << 16, not an offset inside the short last block (only the end of the last run ever takes it: bi_p2v)
ARX_HDI uint64_t bi_p2v(const int64_t *at, uint64_t p_total, uint64_t v_total, uint64_t p) { return p == p_total ? v_total : (uint64_t)at[p >> 16] << 16 | (p & 0xffff); }
struct BiXlatF {
	uint64_t *lin; const int64_t *at; uint64_t p_total, v_total;
	ARX_DEVI void operator()(int64_t i) const { if (lin[i] != BI_UNSET) lin[i] = bi_p2v(at, p_total, v_total, lin[i]); }
};
// ((uint32_t)refID, pos) in one word that orders as the pair does, pos as the signed number it is
ARX_HDI uint64_t bi_key(const uint8_t *p) { return (uint64_t)bs_r32(p + 4) << 32 | (uint64_t)(bs_r32(p + 8) ^ 0x80000000u); }
ARX_HDI int bi_key_bits(int32_t n_ref, const BiScheme &sc) { return bs_key_bits(n_ref) - 32 + sc.bin_bits(); } // of refID << bin_bits | bin, refID up to n_ref

// the last record found in an open buffer: whole (its fixed part, name and CIGAR are here, or all of it where block_size says less) or carried
struct BiTailF {
	const uint8_t *s; int64_t n; const int64_t *rec_off; int64_t n_found; int64_t *words;
	ARX_DEVI void operator()(int64_t) const
	{
		const int64_t o = rec_off[n_found - 1], avail = n - o;
		bool whole = avail >= 36;
		if (whole) {
			const uint8_t *p = s + o;
			const int64_t all = 4 + (int64_t)bs_r32(p), need = 36 + (int64_t)p[12] + 4 * ((int64_t)p[16] | (int64_t)p[17] << 8);
			whole = avail >= (need < all ? need : all);
		}
		words[BI_W_NP] = whole ? n_found : n_found - 1;
		words[BI_W_FROM] = whole ? rec_off[n_found] : o;
	}
};

struct BiRecF {
	const uint8_t *s; int64_t n; const int64_t *rec_off; BiOff off;
	int32_t n_ref; const int32_t *ref_len; const int64_t *lin_base; uint64_t *lin;
	int64_t rec0;                      // the number of the buffer's first record
	uint64_t *rb, *vbeg; int64_t *cnt; // per record: refID << bin_bits | bin; V(start) (P(start) under the closed form); mapped | unmapped << 32
	int64_t *words;
	BiScheme sc;
	ARX_DEVI void fail(int64_t j, int rule) const { ARX_ATOMIC_MINU64((uint64_t *)&words[BI_W_ERR], (uint64_t)(rec0 + j) << 8 | (uint64_t)rule); }
	ARX_DEVI void operator()(int64_t j) const
	{
		const int64_t o = rec_off[j];
		const uint8_t *p = s + o; // at least 36 bytes: bi_run hands over whole records only
		const int bits = sc.bin_bits();
		rb[j] = (uint64_t)(uint32_t)n_ref << bits; cnt[j] = 0;
		vbeg[j] = bi_off(off, o);
		const int64_t all = 4 + (int64_t)bs_r32(p), l_name = p[12], n_cig = (int64_t)p[16] | (int64_t)p[17] << 8, need = 36 + l_name + 4 * n_cig;
		if (need > all || o + need > n) { fail(j, BI_R_FIELDS); return; }
		const int32_t rid = (int32_t)bs_r32(p + 4), pos = (int32_t)bs_r32(p + 8);
		const uint32_t flag = (uint32_t)p[18] | (uint32_t)p[19] << 8;
		if (rid < -1 || rid >= n_ref) { fail(j, BI_R_REFID); return; }
		if (rid < 0) return; // no coordinate: counted by what the count words leave
		if (pos < 0) { fail(j, BI_R_POS); return; }
		int64_t len = 0;
		if (!(flag & 4)) {
			const uint8_t *c = p + 36 + l_name;
			for (int64_t k = 0; k < n_cig; ++k) {
				const uint32_t w = bs_r32(c + 4 * k), op = w & 15;
				if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) len += (int64_t)(w >> 4);
			}
		}
		const int64_t beg = pos, end = beg + (len > 0 ? len : 1);
		if (end > (int64_t)ref_len[rid]) { fail(j, BI_R_END); return; }
		rb[j] = (uint64_t)(uint32_t)rid << bits | sc.bin(beg, end);
		cnt[j] = flag & 4 ? (int64_t)1 << 32 : 1;
		const uint64_t v = vbeg[j];
		uint64_t *win = lin + lin_base[rid]; // end <= ref_len: every window lies in the contig's part of the table
		for (int64_t w = beg >> sc.min_shift; w <= (end - 1) >> sc.min_shift; ++w)
			if (ARX_LOAD_SHARED(&win[w]) > v) ARX_ATOMIC_MINU64(&win[w], v); // (values only fall: a read that is too old is too large, and the minimum is taken)
	}
};

struct BiFlagF {
	const uint8_t *s; const int64_t *rec_off; const uint64_t *rb; int64_t np, rec0;
	int32_t n_ref, have_prev; uint64_t prev_key, prev_rb; // the last record of the buffers before
	int64_t *flag, *words;
	BiScheme sc;
	ARX_DEVI void operator()(int64_t j) const
	{
		const uint64_t key = bi_key(s + rec_off[j]);
		const bool has = j > 0 || have_prev;
		const uint64_t kp = j > 0 ? bi_key(s + rec_off[j - 1]) : prev_key, rp = j > 0 ? rb[j - 1] : prev_rb;
		if (has && key < kp) ARX_ATOMIC_MINU64((uint64_t *)&words[BI_W_ERR], (uint64_t)(rec0 + j) << 8 | (uint64_t)BI_R_ORDER);
		const bool same = has && rb[j] == rp;
		flag[j] = j == 0 || !same; // a buffer's first record opens a run of its own: the host joins it to the one it continues
		if (!same && (rb[j] >> sc.bin_bits()) < (uint64_t)(uint32_t)n_ref) ARX_ATOMIC_ADD64(&words[BI_W_RUNS], 1);
		if (j == 0) words[BI_W_CONT] = same;
		if (j == np - 1) { words[BI_W_LASTKEY] = (int64_t)key; words[BI_W_LASTRB] = (int64_t)rb[j]; }
	}
};

struct BiRunCols { uint64_t *key, *beg, *end; int64_t *c0; uint32_t *idx; }; // n_runs each, c0: n_runs + 1 -- the count words in front of a run
struct BiRunsF {
	const int64_t *flag, *fx, *cx; const uint64_t *rb, *vbeg; int64_t np; uint64_t vend_last; BiRunCols r;
	ARX_DEVI void operator()(int64_t j) const
	{
		if (flag[j]) {
			const int64_t k = fx[j];
			r.key[k] = rb[j]; r.beg[k] = vbeg[j]; r.c0[k] = cx[j]; r.idx[k] = (uint32_t)k;
			if (k > 0) r.end[k - 1] = vbeg[j];
		}
		if (j == np - 1) { r.end[fx[np] - 1] = vend_last; r.c0[fx[np]] = cx[np]; }
	}
};
struct BiHeadF { // i: a run in sorted order
	const uint64_t *skey; const uint32_t *idx; BiRunCols r; int64_t *head, *cs;
	ARX_DEVI void operator()(int64_t i) const
	{
		const uint32_t v = idx[i];
		cs[i] = r.c0[v + 1] - r.c0[v]; // (both halves grow: no borrow)
		head[i] = i == 0 || skey[i] != skey[i - 1] || (r.end[idx[i - 1]] >> 16) < (r.beg[v] >> 16);
	}
};
struct BiChunkCols { uint64_t *key, *beg, *end; int64_t *c0; }; // n_chunks each, c0: n_chunks + 1
struct BiChunksF {
	const uint64_t *skey; const uint32_t *idx; BiRunCols r; const int64_t *head, *hx, *sx; int64_t n_runs; BiChunkCols c;
	ARX_DEVI void operator()(int64_t i) const
	{
		if (head[i]) {
			const int64_t k = hx[i];
			c.key[k] = skey[i]; c.beg[k] = r.beg[idx[i]]; c.c0[k] = sx[i];
			if (k > 0) c.end[k - 1] = r.end[idx[i - 1]];
		}
		if (i == n_runs - 1) { c.end[hx[n_runs] - 1] = r.end[idx[i]]; c.c0[hx[n_runs]] = sx[n_runs]; }
	}
};

// ---- the host's side
// the file's block table: the non-empty blocks with where their bytes start in the inflated stream, and the slabs
struct BiBlocks {
	std::vector<int64_t> ooff, at; // the non-empty blocks, and one entry more: (total, the first block behind the last non-empty one, else the file's end)
	std::vector<int64_t> cut_b, cut_o; // slab k: the blocks [cut_b[k], cut_b[k + 1]), the stream's bytes [cut_o[k], cut_o[k + 1])
	int64_t total = 0;
	int64_t n_slabs() const { return (int64_t)cut_b.size() - 1; }
	// false: a file offset of 2^48 or more
	bool build(int64_t n_blocks, const int64_t *blk_at, const int32_t *isize, int64_t slab_max)
	{
		int64_t end_at = blk_at[n_blocks], in_slab = 0;
		cut_b.assign(1, 0); cut_o.assign(1, 0);
		for (int64_t b = 0; b < n_blocks; ++b) {
			if (in_slab > 0 && slab_max > 0 && in_slab + isize[b] > slab_max) { cut_b.push_back(b); cut_o.push_back(total); in_slab = 0; }
			if (isize[b] > 0) { ooff.push_back(total); at.push_back(blk_at[b]); end_at = blk_at[b + 1]; }
			in_slab += isize[b]; total += isize[b];
		}
		if (n_blocks > 0) { cut_b.push_back(n_blocks); cut_o.push_back(total); }
		ooff.push_back(total); at.push_back(end_at);
		for (int64_t b = 0; b <= n_blocks; ++b)
			if (blk_at[b] < 0 || blk_at[b] >= BI_MAX_AT) return false;
		return true;
	}
	int64_t row_of(int64_t o) const // the last row that starts at or before o
	{
		int64_t lo = 0, hi = (int64_t)ooff.size();
		while (hi - lo > 1) {
			const int64_t mid = lo + (hi - lo) / 2;
			if (ooff[(size_t)mid] <= o) lo = mid; else hi = mid;
		}
		return lo;
	}
	uint64_t voff(int64_t o) const // V(o), o <= total
	{
		if (o >= total) return (uint64_t)at.back() << 16;
		const int64_t r = row_of(o);
		return (uint64_t)at[(size_t)r] << 16 | (uint64_t)(o - ooff[(size_t)r]);
	}
};

struct BiChunk { uint64_t beg, end; };
struct BiRef {
	std::map<uint32_t, std::vector<BiChunk> > bins;
	uint64_t vmin = BI_UNSET, vmax = 0; // V(the first record), the end of the last
	int64_t n_mapped = 0, n_unmapped = 0;
	std::vector<uint64_t> lin;
};
struct BiIndex {
	BiScheme sc = BI_BAI;
	std::vector<BiRef> refs;
	int64_t n_no_coor = 0, n_records = 0, n_slabs = 0, n_runs = 0, n_chunks = 0, n_bins = 0, n_lin = 0;
	uint64_t err = BI_UNSET; // BI_E_RULE: the first offending record's number << 8 | the rule
};

// a slab's joined chunks, in (refID, bin) order and file order within: appended bin by bin, joined to the bin's last by the rule of the device
inline void bi_append(BiIndex &ix, int32_t n_ref, const uint64_t *key, const uint64_t *beg, const uint64_t *end, const int64_t *c0, int64_t n)
{
	const int bits = ix.sc.bin_bits();
	for (int64_t k = 0; k < n; ++k) {
		const uint64_t ref = key[k] >> bits;
		if (ref >= (uint64_t)n_ref) continue; // the records without a coordinate
		BiRef &r = ix.refs[(size_t)ref];
		std::vector<BiChunk> &v = r.bins[(uint32_t)(key[k] & (((uint64_t)1 << bits) - 1))];
		if (!v.empty() && (v.back().end >> 16) >= (beg[k] >> 16)) v.back().end = end[k];
		else v.push_back(BiChunk{beg[k], end[k]});
		const int64_t c = c0[k + 1] - c0[k];
		r.n_mapped += c & 0xffffffff; r.n_unmapped += c >> 32;
		if (beg[k] < r.vmin) r.vmin = beg[k];
		if (end[k] > r.vmax) r.vmax = end[k];
	}
}

// the first contig the BAI format cannot hold, or -1: bi_run's callers refuse such a header
inline int32_t bi_long_contig(int32_t n_ref, const int32_t *ref_len)
{
	for (int32_t i = 0; i < n_ref; ++i)
		if ((int64_t)ref_len[i] > BI_MAX_REF) return i;
	return -1;
}
inline int64_t bi_windows(int32_t len, int min_shift) { return len > 0 ? ((int64_t)len + (((int64_t)1 << min_shift) - 1)) >> min_shift : 0; }
// a CSI index's min_shift as used (0: 14), or -1 where it lies outside [10, 24]
inline int32_t bi_csi_shift(int32_t min_shift)
{
	if (min_shift == 0) return BI_CSI_SHIFT_DEFAULT;
	return min_shift >= BI_CSI_SHIFT_MIN && min_shift <= BI_CSI_SHIFT_MAX ? min_shift : -1;
}
// a CSI index's scheme for a header: the smallest depth, from the BAI's 5 on, at which bin 0 spans the longest contig.  No shallower than the
// BAI's, so that at min_shift 14 every header the BAI can hold keeps the BAI's bins; 2^31 - 1 bases at min_shift 10 give the deepest, 7
inline BiScheme bi_csi_scheme(int32_t min_shift, int32_t n_ref, const int32_t *ref_len)
{
	int64_t longest = 0;
	for (int32_t i = 0; i < n_ref; ++i)
		if (ref_len[i] > longest) longest = ref_len[i];
	BiScheme sc = {min_shift, BI_BAI.depth};
	while (((int64_t)1 << (sc.min_shift + 3 * sc.depth)) < longest) ++sc.depth;
	return sc;
}

// The slab body, stated once: bi_run pulls its slabs from a source, BiPush is handed them.  begin(); slab() for the stream's bytes [a, b) in
// order; table() at the end.  sc: the bin scheme, bin 0 of which spans every contig (BI_BAI: contigs of at most BI_MAX_REF bases); seg as in dev_bamsort.h
template <class Drv> struct BiSlabs {
	typedef typename Drv::Buf Buf;
	BiIndex *ix = nullptr;
	int32_t n_ref = 0;
	int64_t seg = 0, L = 0;
	BiScheme sc = BI_BAI;
	std::vector<int64_t> base;
	Buf d_lin, d_base, d_len, d_words, buf, next, d_segs, d_off, d_rows, d_rec, d_scan, d_runs, d_chunks;
	int64_t entry = 0, g0 = 0, carry = 0, from = 0; // the buffer's first `carry` bytes are the last buffer's from `from` on
	int32_t have_prev = 0;
	uint64_t prev_key = 0, prev_rb = 0;

	void begin(Drv &drv, BiIndex &x, int64_t hdr, int32_t n_ref_, const int32_t *ref_len, int64_t seg_, const BiScheme &sc_)
	{
		ix = &x; n_ref = n_ref_; seg = seg_; sc = sc_;
		x = BiIndex();
		x.sc = sc;
		x.refs.resize((size_t)n_ref);
		base.assign((size_t)n_ref + 1, 0);
		for (int32_t i = 0; i < n_ref; ++i) base[(size_t)i + 1] = base[(size_t)i] + bi_windows(ref_len[i], sc.min_shift);
		L = base[(size_t)n_ref];
		d_lin.alloc((size_t)L * 8);
		if (L) drv.fill(d_lin.p, 0xff, (size_t)L * 8);
		d_base.alloc(base.size() * 8);
		drv.upload(d_base.p, base.data(), base.size() * 8);
		d_len.alloc((size_t)n_ref * 4);
		if (n_ref) drv.upload(d_len.p, ref_len, (size_t)n_ref * 4);
		d_words.alloc(BI_N_WORDS * 8);
		drv.fill(d_words.p, 0, BI_N_WORDS * 8);
		drv.put(&d_words.template as<int64_t>()[BI_W_ERR], -1);
		entry = hdr; g0 = carry = from = 0; have_prev = 0; prev_key = prev_rb = 0;
	}

	// the stream's bytes [a, b), behind those of the call before.  load(dst): puts them at dst (false: BI_E_INFLATE); off(g0, b, d_rows): the BiOff of
	// a buffer that holds the stream's [g0, b); vend(o): the offset word of the stream's byte o <= b.  closed: the chain ends with b
	template <class Load, class Off, class End> int slab(Drv &drv, int64_t a, int64_t b, bool closed, Load load, Off off, End vend)
	{
		int64_t *words = d_words.template as<int64_t>();
		const int64_t n = carry + (b - a);
		next.alloc((size_t)n);
		if (carry) drv.copy(next.p, buf.template as<uint8_t>() + from, (size_t)carry);
		if (!load(next.template as<uint8_t>() + carry)) return BI_E_INFLATE;
		std::swap(buf, next);
		next.release();
		g0 = a - carry;
		const uint8_t *s = buf.template as<uint8_t>();
		const BsStream t = {s, n, entry - g0, seg, n_ref, closed ? 0 : 1};
		const int64_t ns = bs_n_seg(t);
		d_segs.alloc((size_t)bs_seg_words(ns) * 8);
		BsSegs w; w.carve(d_segs.template as<int64_t>(), ns);
		BsFound f;
		if (bs_discover(drv, t, w, &f) != BS_OK) return BI_E_CHAIN;
		d_off.alloc((size_t)(f.n_records + 1) * 8);
		int64_t *rec_off = d_off.template as<int64_t>();
		bs_fill(drv, t, w, f, rec_off);
		int64_t np = f.n_records;
		from = f.exit;
		if (!closed && f.n_records > 0) {
			drv.items("bi_tail", 1, BiTailF{s, n, rec_off, f.n_records, words});
			np = drv.get(&words[BI_W_NP]); from = drv.get(&words[BI_W_FROM]);
		}
		++ix->n_slabs;
		if (np > 0) {
			const BiOff R = off(g0, b, d_rows);
			d_rec.alloc((size_t)np * 8 * 4);
			uint64_t *rb = d_rec.template as<uint64_t>(), *vbeg = rb + np;
			int64_t *cnt = (int64_t *)(vbeg + np), *flag = cnt + np;
			d_scan.alloc((size_t)(np + 1) * 8 * 2);
			int64_t *fx = d_scan.template as<int64_t>(), *cx = fx + np + 1;
			drv.items("bi_rec", np, BiRecF{s, n, rec_off, R, n_ref, d_len.template as<int32_t>(), d_base.template as<int64_t>(), d_lin.template as<uint64_t>(), ix->n_records, rb, vbeg, cnt, words, sc});
			drv.items("bi_flag", np, BiFlagF{s, rec_off, rb, np, ix->n_records, n_ref, have_prev, prev_key, prev_rb, flag, words, sc});
			const uint64_t err = (uint64_t)drv.get(&words[BI_W_ERR]);
			if (err != BI_UNSET) { ix->err = err; return BI_E_RULE; }
			drv.scan(flag, fx, np, "bi_scan");
			drv.scan(cnt, cx, np, "bi_scan");
			const int64_t n_runs = drv.get(&fx[np]), placed = drv.get(&cx[np]);
			ix->n_no_coor += np - (placed & 0xffffffff) - (placed >> 32);
			prev_key = (uint64_t)drv.get(&words[BI_W_LASTKEY]); prev_rb = (uint64_t)drv.get(&words[BI_W_LASTRB]); have_prev = 1;
			// runs, then chunks
			d_runs.alloc((size_t)n_runs * (8 * 5 + 4 * 2) + (size_t)(n_runs + 1) * 8 * 4);
			uint64_t *q = d_runs.template as<uint64_t>();
			BiRunCols rc; uint64_t *skey; int64_t *head, *cs, *hx, *sx; uint32_t *idx;
			rc.key = q; q += n_runs; rc.beg = q; q += n_runs; rc.end = q; q += n_runs; skey = q; q += n_runs;
			head = (int64_t *)q; q += n_runs; rc.c0 = (int64_t *)q; q += n_runs + 1; cs = (int64_t *)q; q += n_runs + 1; hx = (int64_t *)q; q += n_runs + 1;
			sx = (int64_t *)q; q += n_runs + 1; rc.idx = (uint32_t *)q; idx = rc.idx + n_runs;
			drv.items("bi_runs", np, BiRunsF{flag, fx, cx, rb, vbeg, np, vend(g0 + from), rc});
			drv.sort_pairs(rc.key, skey, rc.idx, idx, n_runs, bi_key_bits(n_ref, sc));
			drv.items("bi_head", n_runs, BiHeadF{skey, idx, rc, head, cs});
			drv.scan(head, hx, n_runs, "bi_scan");
			drv.scan(cs, sx, n_runs, "bi_scan");
			const int64_t n_ch = drv.get(&hx[n_runs]);
			d_chunks.alloc((size_t)(4 * n_ch + 1) * 8);
			uint64_t *u = d_chunks.template as<uint64_t>();
			const BiChunkCols cc = {u, u + n_ch, u + 2 * n_ch, (int64_t *)(u + 3 * n_ch)};
			drv.items("bi_chunks", n_runs, BiChunksF{skey, idx, rc, head, hx, sx, n_runs, cc});
			std::vector<uint64_t> h((size_t)(4 * n_ch + 1));
			drv.fetch(h.data(), d_chunks.p, h.size() * 8);
			bi_append(*ix, n_ref, h.data(), h.data() + n_ch, h.data() + 2 * n_ch, (const int64_t *)(h.data() + 3 * n_ch), n_ch);
			ix->n_records += np;
		}
		entry = g0 + from;
		carry = from < n ? n - from : 0;
		return BI_OK;
	}

	// the linear index: cut behind the highest window set, an unset window below takes the next set one's value.  xlat(lin, L): what is still to
	// be done to the table where it lies (BiPush: P -> V)
	template <class Xlat> void table(Drv &drv, Xlat xlat)
	{
		ix->n_runs = drv.get(&d_words.template as<int64_t>()[BI_W_RUNS]);
		if (L) xlat(d_lin.template as<uint64_t>(), L);
		std::vector<uint64_t> lin((size_t)L);
		if (L) drv.fetch(lin.data(), d_lin.p, (size_t)L * 8);
		for (int32_t i = 0; i < n_ref; ++i) {
			BiRef &r = ix->refs[(size_t)i];
			const uint64_t *win = lin.data() + base[(size_t)i];
			int64_t hi = base[(size_t)i + 1] - base[(size_t)i] - 1;
			while (hi >= 0 && win[hi] == BI_UNSET) --hi;
			r.lin.assign(win, win + (hi + 1));
			for (int64_t x = hi - 1; x >= 0; --x)
				if (r.lin[(size_t)x] == BI_UNSET) r.lin[(size_t)x] = r.lin[(size_t)x + 1];
			ix->n_lin += hi + 1;
			ix->n_bins += (int64_t)r.bins.size();
			for (const auto &bn : r.bins) ix->n_chunks += (int64_t)bn.second.size();
		}
	}
};

// -> BI_*.  BI_E_RULE: ix.err says which record and rule.  ix.refs[i].lin is the table of windows of 2^sc.min_shift bases, cut and backfilled
template <class Drv, class Src> int bi_run(Drv &drv, Src &src, const BiBlocks &B, int64_t hdr, int32_t n_ref, const int32_t *ref_len, int64_t seg, BiIndex &ix, const BiScheme sc = BI_BAI)
{
	typedef typename Drv::Buf Buf;
	BiSlabs<Drv> S;
	S.begin(drv, ix, hdr, n_ref, ref_len, seg, sc);
	const int64_t n_slabs = B.n_slabs();
	for (int64_t k = 0; k < n_slabs; ++k) {
		const int64_t a = B.cut_o[(size_t)k], b = B.cut_o[(size_t)k + 1];
		const int rc = S.slab(drv, a, b, k + 1 == n_slabs, [&](uint8_t *dst) { return src.load(k, dst, b - a); },
		                      [&](int64_t g0, int64_t b_, Buf &d_rows) { // the rows of the blocks the buffer's bytes lie in
			const int64_t r0 = B.row_of(g0), r1 = B.row_of(b_ - 1) + 1;
			std::vector<int64_t> rows((size_t)(2 * (r1 - r0)));
			for (int64_t r = r0; r < r1; ++r) { rows[(size_t)(r - r0)] = B.ooff[(size_t)r] - g0; rows[(size_t)(r1 - r0 + r - r0)] = B.at[(size_t)r]; }
			d_rows.alloc(rows.size() * 8);
			drv.upload(d_rows.p, rows.data(), rows.size() * 8);
			return BiOff{BiRows{d_rows.template as<int64_t>(), d_rows.template as<int64_t>() + (r1 - r0), r1 - r0}, 0, 0};
		}, [&](int64_t o) { return B.voff(o); });
		if (rc != BI_OK) return rc;
	}
	if (n_slabs == 0 && hdr != B.total) return BI_E_CHAIN;
	S.table(drv, [](uint64_t *, int64_t) {});
	return BI_OK;
}

// bi_run with the direction reversed, for a writer that is handed its record stream piece by piece (the bytes behind the header; they end
// anywhere -- inside a block_size field, the fixed part, a CIGAR: discovery with an open end, bi_tail and the carry see to that):
// begin(), feed() any number of times, finish() with the table of the blocks the writer wrote.  Until then every offset is P (above).
// Memory on top of the caller's bytes: the window table for the writer's life, and per feed one piece at a time -- the piece's bytes with the carry in
// front, 56 bytes per record of the piece, about 100 per run; finish() adds 8 bytes per block for as long as it runs
template <class Drv> struct BiPush {
	BiSlabs<Drv> S;
	BiIndex ix;
	int64_t hb = 0, total = 0, piece = 0;
	typename Drv::Buf d_at;

	// H: the header's bytes in front of the record stream; piece_max: the most bytes of a feed indexed at once (0: all of them)
	void begin(Drv &drv, int32_t n_ref, const int32_t *ref_len, const BiScheme &sc, int64_t H, int64_t seg, int64_t piece_max)
	{
		S.begin(drv, ix, 0, n_ref, ref_len, seg, sc);
		hb = bi_header_blocks(H); total = 0; piece = piece_max;
	}
	// d[0, n): the next bytes of the record stream, in the launches' memory -> BI_*.  After anything but BI_OK the index is lost
	int feed(Drv &drv, const uint8_t *d, int64_t n)
	{
		for (int64_t o = 0; o < n;) {
			const int64_t len = piece > 0 && n - o > piece ? piece : n - o, a = total;
			const int rc = S.slab(drv, a, a + len, false, [&](uint8_t *dst) { drv.copy(dst, d + o, (size_t)len); return true; },
			                      [&](int64_t g0, int64_t, typename Drv::Buf &) { return BiOff{BiRows{nullptr, nullptr, 0}, g0, hb}; }, [&](int64_t at) { return bi_poff(hb, at); });
			if (rc != BI_OK) return rc;
			total += len; o += len;
		}
		return BI_OK;
	}
	int64_t n_blocks() const { return hb + (total + BI_BLOCK - 1) / BI_BLOCK; } // of the writer's layout, the EOF block not counted
	// at[0 .. n_blocks()]: where the blocks lie in the file, the last entry the EOF block's -> BI_OK, or BI_E_CHAIN: the stream ends inside a record
	int finish(Drv &drv, const int64_t *at)
	{
		if (S.carry != 0 || S.entry != total) return BI_E_CHAIN;
		const int64_t nb = n_blocks();
		const uint64_t p_total = bi_poff(hb, total), v_total = (uint64_t)at[nb] << 16;
		S.table(drv, [&](uint64_t *lin, int64_t L) {
			d_at.alloc((size_t)(nb + 1) * 8);
			drv.upload(d_at.p, at, (size_t)(nb + 1) * 8);
			drv.items("bi_xlat", L, BiXlatF{lin, d_at.template as<int64_t>(), p_total, v_total});
		});
		d_at.release();
		for (BiRef &r : ix.refs) {
			for (auto &bn : r.bins)
				for (BiChunk &c : bn.second) { c.beg = bi_p2v(at, p_total, v_total, c.beg); c.end = bi_p2v(at, p_total, v_total, c.end); }
			if (r.vmin != BI_UNSET) { r.vmin = bi_p2v(at, p_total, v_total, r.vmin); r.vmax = bi_p2v(at, p_total, v_total, r.vmax); }
		}
		return BI_OK;
	}
};

// the bytes of the .bai (the SAM specification, 5.2): bins ascending, the pseudo-bin last in every contig that holds a record, n_no_coor always
inline std::vector<uint8_t> bi_serialise(const BiIndex &ix)
{
	std::vector<uint8_t> o;
	auto put = [&](uint64_t v, int bytes) { for (int k = 0; k < bytes; ++k) o.push_back((uint8_t)(v >> (8 * k))); };
	o.push_back('B'); o.push_back('A'); o.push_back('I'); o.push_back(1);
	put((uint64_t)ix.refs.size(), 4);
	for (const BiRef &r : ix.refs) {
		const bool any = r.n_mapped + r.n_unmapped > 0;
		put((uint64_t)r.bins.size() + (any ? 1 : 0), 4);
		for (const auto &bn : r.bins) {
			put(bn.first, 4); put((uint64_t)bn.second.size(), 4);
			for (const BiChunk &c : bn.second) { put(c.beg, 8); put(c.end, 8); }
		}
		if (any) { put(BI_PSEUDO_BIN, 4); put(2, 4); put(r.vmin, 8); put(r.vmax, 8); put((uint64_t)r.n_mapped, 8); put((uint64_t)r.n_unmapped, 8); }
		put((uint64_t)r.lin.size(), 4);
		for (uint64_t v : r.lin) put(v, 8);
	}
	put((uint64_t)ix.n_no_coor, 8);
	return o;
}

// the inflated bytes of the .csi (CSIv1) of an index built under a CSI scheme: bins ascending, each with its loffset -- the value of the first
// window of its interval in the backfilled table, which a record of the bin has set at or behind it --, the meta-bin last in every contig that
// holds a record, no aux block, no linear index, n_no_coor always.  Tens to thousands of bins: the lookup is the host's
inline std::vector<uint8_t> bi_serialise_csi(const BiIndex &ix)
{
	std::vector<uint8_t> o;
	auto put = [&](uint64_t v, int bytes) { for (int k = 0; k < bytes; ++k) o.push_back((uint8_t)(v >> (8 * k))); };
	o.push_back('C'); o.push_back('S'); o.push_back('I'); o.push_back(1);
	put((uint64_t)ix.sc.min_shift, 4); put((uint64_t)ix.sc.depth, 4); put(0, 4);
	put((uint64_t)ix.refs.size(), 4);
	for (const BiRef &r : ix.refs) {
		const bool any = r.n_mapped + r.n_unmapped > 0;
		put((uint64_t)r.bins.size() + (any ? 1 : 0), 4);
		for (const auto &bn : r.bins) {
			put(bn.first, 4); put(r.lin[(size_t)ix.sc.first_window(bn.first)], 8); put((uint64_t)bn.second.size(), 4);
			for (const BiChunk &c : bn.second) { put(c.beg, 8); put(c.end, 8); }
		}
		if (any) { put(ix.sc.meta(), 4); put(0, 8); put(2, 4); put(r.vmin, 8); put(r.vmax, 8); put((uint64_t)r.n_mapped, 8); put((uint64_t)r.n_unmapped, 8); }
	}
	put((uint64_t)ix.n_no_coor, 8);
	return o;
}

// the text of a refusal: the record's number (from 0, in file order) and the rule
inline std::string bi_rule_text(uint64_t err)
{
	static const char *rule[] = {"", "its name and CIGAR do not fit into its block_size", "its refID lies outside [-1, n_ref)", "it has a refID but pos < 0",
	                             "its end lies beyond the length of its contig", "its key ((uint32_t)refID, pos) is smaller than its predecessor's: the file is not sorted by coordinate"};
	const uint64_t r = err & 0xff;
	return "record " + std::to_string(err >> 8) + ": " + (r >= 1 && r <= 5 ? rule[r] : "unknown rule");
}

} // namespace arx

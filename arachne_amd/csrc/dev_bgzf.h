// dev_bgzf.h -- one BGZF block (at most 65280 input bytes) -> one raw DEFLATE stream (RFC 1951) plus the CRC-32 of the input, as phases over
// an explicit lane index.  hip_bgzf.h runs the phases with one workgroup of BGZF_LANES lanes per block and a barrier where a phase ends;
// tests/bgzfsim/bgzf_sim.cpp runs the very same functions on the host, lanes in a loop.  Nothing here knows which of the two it is.
//
// What a block goes through (bgzf_block):
//   load       the input into work memory, the hash heads and histograms cleared
//   candidates in chunks of BGZF_CHUNK positions: every position of the chunk READS the head of its hash (the largest position of any
//              EARLIER chunk with the same 4-byte hash), a barrier, then every position of the chunk is inserted with an atomic max.  The
//              head a position sees is a function of the input alone, whatever order the lanes run in
//   parse      lane l owns positions [l * BGZF_SUB, (l + 1) * BGZF_SUB): a greedy parse, every candidate verified byte by byte, a second
//              candidate at distance 1 (runs), matches cut at the end of the lane's range; tokens go where the candidates were, symbol
//              counts into the two histograms (atomic adds: sums do not depend on their order)
//   crc        table-driven CRC-32 of every lane's range, shifted by x^(8 * bytes behind the range) mod P and xor-ed (what zlib's
//              crc32_combine does pairwise); the shifts over whole lane ranges are tabulated once per workgroup
//   codes      length-limited Huffman codes of the literal/length and distance alphabets (15 bits) and, over their lengths, of the code
//              length alphabet (7 bits): symbols ranked by (count, symbol) in parallel, then one lane per tree runs the in-place
//              minimum-redundancy construction of Moffat and Katajainen on the sorted counts and moves leaves down until the Kraft sum
//              is exactly 1 under the limit
//   decide     exact bit counts of the dynamic form, the fixed form and the stored form from the histograms; the smallest is emitted
//   emit       bits per lane -> exclusive scan -> every lane writes its tokens at its bit offset into the zeroed output: whole words it
//              owns with plain stores, the first and the last word it touches with an atomic or
// Every loop is bounded by the block length or an alphabet size; no lane waits for another one outside the barriers between phases.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include "arx_dev.h"
#define ARX_BGZF_MAX(p, v) atomicMax((unsigned int *)(p), (unsigned int)(v))
#define ARX_BGZF_ADD(p, v) atomicAdd((unsigned int *)(p), (unsigned int)(v))
#define ARX_BGZF_OR(p, v) atomicOr((unsigned int *)(p), (unsigned int)(v))
#else
#include "arx_hd.h"
#define ARX_BGZF_MAX(p, v) (*(p) = *(p) > (uint32_t)(v) ? *(p) : (uint32_t)(v))
#define ARX_BGZF_ADD(p, v) (*(p) += (uint32_t)(v))
#define ARX_BGZF_OR(p, v) (*(p) |= (uint32_t)(v))
#endif

namespace arx {

constexpr int BGZF_IN = 0xff00;                   // BamSink::BLOCK_IN
constexpr int BGZF_LANES = 256;                   // lanes of a block's workgroup
constexpr int BGZF_SUB = BGZF_IN / BGZF_LANES;    // 255 positions per lane
constexpr int BGZF_CHUNK = BGZF_LANES;            // positions inserted between two barriers
constexpr int BGZF_HBITS = 12;                    // hash heads
constexpr int BGZF_OUT_SLICE = 65536;             // bytes of a block's output slice; at most 5 + 65280 of them are ever written
constexpr int BGZF_LL = 288, BGZF_D = 32, BGZF_CL = 19; // alphabet sizes (286 and 30 symbols in use)
constexpr int BGZF_MIN_MATCH = 3, BGZF_MAX_MATCH = 258, BGZF_WINDOW = 32768, BGZF_FAR3 = 4096;
enum { BGZF_STORED = 0, BGZF_FIXED = 1, BGZF_DYNAMIC = 2 };
// shared scalars of a block
enum { BZ_MODE = 0, BZ_BITS, BZ_HLIT, BZ_HDIST, BZ_HCLEN, BZ_D_BUMP, BZ_CL_BUMP, BZ_XTAIL, BZ_N_SCALARS };
static_assert(BGZF_SUB * BGZF_LANES == BGZF_IN, "the lanes' ranges tile a full block");

struct BgzfWork {
	uint8_t *in;        // BGZF_IN + 8 bytes, 4-aligned
	uint32_t *head;     // 1 << BGZF_HBITS: position + 1 of the last insertion (0: none)
	uint16_t *tok;      // BGZF_IN + 2: candidates (position + 1), then tokens: 0 = literal, 0x8000 | (distance - 1) followed by the length
	uint32_t *ll_freq, *d_freq, *cl_freq; // BGZF_LL, BGZF_D, BGZF_CL + 1
	uint8_t *ll_len, *d_len, *cl_len;     // code lengths
	uint16_t *ll_code, *d_code, *cl_code; // codes, bit-reversed: ready to be packed LSB first
	uint16_t *order;    // 3 x BGZF_LL: an alphabet's used symbols by ascending (count, symbol)
	uint32_t *tree;     // 3 x BGZF_LL: work array of the construction
	int32_t *cnt;       // 3 x 64: codes per length
	int32_t *bits, *off; // BGZF_LANES and BGZF_LANES + 1: bits per lane, their exclusive scan
	uint32_t *crc_tab;  // 256
	uint32_t *x2n;      // 32: x^(2^k) mod P
	uint32_t *xsub;     // BGZF_LANES: x^(8 * BGZF_SUB * k) mod P, the shift over k whole lane ranges
	uint32_t *crc_part; // BGZF_LANES
	int32_t *sh;        // BZ_N_SCALARS
};
// bytes of work memory behind a BgzfWork, without tok (which is the only array too large for LDS next to the input)
constexpr int BGZF_WORK_BYTES = (BGZF_IN + 8) + 4 * (1 << BGZF_HBITS) + 4 * (BGZF_LL + BGZF_D + BGZF_CL + 1) + (BGZF_LL + BGZF_D + BGZF_CL + 1) +
                                2 * (BGZF_LL + BGZF_D + BGZF_CL + 1) + 2 * 3 * BGZF_LL + 4 * 3 * BGZF_LL + 4 * 3 * 64 + 4 * (2 * BGZF_LANES + 1) +
                                4 * (256 + 32 + 2 * BGZF_LANES) + 4 * BZ_N_SCALARS;

// carves the arrays out of one 4-aligned buffer of BGZF_WORK_BYTES bytes
ARX_DEVI void bgzf_carve(BgzfWork &w, uint8_t *mem, uint16_t *tok)
{
	uint8_t *p = mem;
	w.tok = tok;
	w.in = p; p += BGZF_IN + 8;
	w.head = (uint32_t *)p; p += 4 * (1 << BGZF_HBITS);
	w.ll_freq = (uint32_t *)p; p += 4 * BGZF_LL;
	w.d_freq = (uint32_t *)p; p += 4 * BGZF_D;
	w.cl_freq = (uint32_t *)p; p += 4 * (BGZF_CL + 1);
	w.tree = (uint32_t *)p; p += 4 * 3 * BGZF_LL;
	w.cnt = (int32_t *)p; p += 4 * 3 * 64;
	w.bits = (int32_t *)p; p += 4 * BGZF_LANES;
	w.off = (int32_t *)p; p += 4 * (BGZF_LANES + 1);
	w.crc_tab = (uint32_t *)p; p += 4 * 256;
	w.x2n = (uint32_t *)p; p += 4 * 32;
	w.xsub = (uint32_t *)p; p += 4 * BGZF_LANES;
	w.crc_part = (uint32_t *)p; p += 4 * BGZF_LANES;
	w.sh = (int32_t *)p; p += 4 * BZ_N_SCALARS;
	w.ll_code = (uint16_t *)p; p += 2 * BGZF_LL;
	w.d_code = (uint16_t *)p; p += 2 * BGZF_D;
	w.cl_code = (uint16_t *)p; p += 2 * (BGZF_CL + 1);
	w.order = (uint16_t *)p; p += 2 * 3 * BGZF_LL;
	w.ll_len = p; p += BGZF_LL;
	w.d_len = p; p += BGZF_D;
	w.cl_len = p; p += BGZF_CL + 1;
}

// ---- the alphabets of RFC 1951 3.2.5, computed instead of tabulated
ARX_DEVI int bgzf_log2(uint32_t x) { return 31 - __builtin_clz(x); } // x > 0
ARX_DEVI int bgzf_len_sym(int len, int *eb, int *ev)
{
	if (len == BGZF_MAX_MATCH) { *eb = 0; *ev = 0; return 285; }
	const int l = len - 3;
	if (l < 8) { *eb = 0; *ev = 0; return 257 + l; }
	const int hb = bgzf_log2((uint32_t)l), e = hb - 2;
	*eb = e; *ev = l & ((1 << e) - 1);
	return 261 + 4 * e + ((l >> e) & 3);
}
ARX_DEVI int bgzf_dist_sym(int dist, int *eb, int *ev)
{
	const int d = dist - 1;
	if (d < 4) { *eb = 0; *ev = 0; return d; }
	const int hb = bgzf_log2((uint32_t)d), e = hb - 1;
	*eb = e; *ev = d & ((1 << e) - 1);
	return 2 * hb + ((d >> e) & 1);
}
ARX_DEVI int bgzf_ll_extra(int sym) { return sym < 265 || sym >= 285 ? 0 : (sym - 261) >> 2; }
ARX_DEVI int bgzf_d_extra(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }
ARX_DEVI int bgzf_fixed_ll_len(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }
ARX_DEVI uint32_t bgzf_fixed_ll_code(int sym) { return sym < 144 ? 0x30u + sym : sym < 256 ? 0x190u + (sym - 144) : sym < 280 ? (uint32_t)(sym - 256) : 0xC0u + (sym - 280); }
ARX_DEVI uint32_t bgzf_rev(uint32_t c, int n) // the n low bits of c, reversed
{
	uint32_t r = 0;
	for (int i = 0; i < n; ++i) { r = (r << 1) | (c & 1); c >>= 1; }
	return r;
}
ARX_DEVI uint32_t bgzf_hash(const uint8_t *p)
{
	const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
	return (v * 2654435761u) >> (32 - BGZF_HBITS);
}

// ---- CRC-32 (the reflected polynomial 0xEDB88320 of RFC 1952)
constexpr uint32_t BGZF_POLY = 0xEDB88320u;
ARX_DEVI uint32_t bgzf_gf_mul(uint32_t a, uint32_t b) // a(x) * b(x) mod P, bit 31 = x^0
{
	uint32_t p = 0;
	for (int i = 0; i < 32; ++i) {
		if (a & (0x80000000u >> i)) p ^= b;
		b = (b & 1) ? (b >> 1) ^ BGZF_POLY : b >> 1;
	}
	return p;
}
ARX_DEVI uint32_t bgzf_x8n(const uint32_t *x2n, uint32_t n_bytes) // x^(8 * n_bytes) mod P
{
	uint32_t p = 0x80000000u;
	for (int k = 3; n_bytes; n_bytes >>= 1, ++k)
		if (n_bytes & 1) p = bgzf_gf_mul(x2n[k & 31], p);
	return p;
}
// once per workgroup, before the first block; a barrier after each
ARX_DEV void bgzf_tables(BgzfWork &w, int lane)
{
	for (int i = lane; i < 256; i += BGZF_LANES) {
		uint32_t c = (uint32_t)i;
		for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ BGZF_POLY : c >> 1;
		w.crc_tab[i] = c;
	}
	if (lane == 0) {
		uint32_t p = 0x40000000u; // x^1
		w.x2n[0] = p;
		for (int k = 1; k < 32; ++k) { p = bgzf_gf_mul(p, p); w.x2n[k] = p; }
	}
}
// the operators of the fixed range length: what is behind a lane's range is some whole ranges and the block's last, shorter one
ARX_DEV void bgzf_shift_table(BgzfWork &w, int lane) { w.xsub[lane] = bgzf_x8n(w.x2n, (uint32_t)(BGZF_SUB * lane)); }

// ---- phases of one block; n = its input bytes (1 .. BGZF_IN)
ARX_DEV void bgzf_load(BgzfWork &w, const uint8_t *src, int n, int lane)
{
	if (((uintptr_t)src & 3) == 0) {
		const uint32_t *s4 = (const uint32_t *)src;
		uint32_t *d4 = (uint32_t *)w.in;
		for (int i = lane; i < (n >> 2); i += BGZF_LANES) d4[i] = s4[i];
		for (int i = (n & ~3) + lane; i < n; i += BGZF_LANES) w.in[i] = src[i];
	} else
		for (int i = lane; i < n; i += BGZF_LANES) w.in[i] = src[i];
	for (int i = lane; i < (1 << BGZF_HBITS); i += BGZF_LANES) w.head[i] = 0;
	for (int i = lane; i < BGZF_LL; i += BGZF_LANES) w.ll_freq[i] = 0;
	for (int i = lane; i < BGZF_D; i += BGZF_LANES) w.d_freq[i] = 0;
	for (int i = lane; i < BGZF_CL + 1; i += BGZF_LANES) w.cl_freq[i] = 0;
	if (lane == 0) {
		w.ll_freq[256] = 1; // the end-of-block symbol
		const int last = (n - 1) / BGZF_SUB; // the last lane with input; its range has n - last * BGZF_SUB bytes
		w.sh[BZ_XTAIL] = (int32_t)bgzf_x8n(w.x2n, (uint32_t)(n - last * BGZF_SUB));
	}
}
ARX_DEV void bgzf_cand_read(BgzfWork &w, int n, int chunk, int lane)
{
	for (int p = chunk * BGZF_CHUNK + lane; p < (chunk + 1) * BGZF_CHUNK && p < n; p += BGZF_LANES)
		w.tok[p] = p + 4 <= n ? (uint16_t)w.head[bgzf_hash(w.in + p)] : (uint16_t)0;
}
ARX_DEV void bgzf_cand_insert(BgzfWork &w, int n, int chunk, int lane)
{
	for (int p = chunk * BGZF_CHUNK + lane; p < (chunk + 1) * BGZF_CHUNK && p + 4 <= n; p += BGZF_LANES)
		ARX_BGZF_MAX(&w.head[bgzf_hash(w.in + p)], p + 1);
}
ARX_DEV void bgzf_parse(BgzfWork &w, int n, int lane)
{
	const int s = lane * BGZF_SUB, e = s + BGZF_SUB < n ? s + BGZF_SUB : n;
	const uint8_t *in = w.in;
	for (int p = s; p < e;) {
		const int maxl = e - p < BGZF_MAX_MATCH ? e - p : BGZF_MAX_MATCH;
		int best = 0, bdist = 0;
		if (maxl >= BGZF_MIN_MATCH) {
			const int c = w.tok[p];
			if (c && p - (c - 1) <= BGZF_WINDOW) {
				const int q = c - 1;
				int l = 0;
				while (l < maxl && in[q + l] == in[p + l]) ++l;
				if (l >= BGZF_MIN_MATCH && !(l == BGZF_MIN_MATCH && p - q > BGZF_FAR3)) { best = l; bdist = p - q; }
			}
			if (p > 0 && in[p - 1] == in[p]) {
				int l = 1;
				while (l < maxl && in[p + l] == in[p - 1]) ++l;
				if (l >= BGZF_MIN_MATCH && l >= best) { best = l; bdist = 1; }
			}
		}
		if (best) {
			int eb, ev;
			w.tok[p] = (uint16_t)(0x8000 | (bdist - 1));
			w.tok[p + 1] = (uint16_t)best;
			ARX_BGZF_ADD(&w.ll_freq[bgzf_len_sym(best, &eb, &ev)], 1);
			ARX_BGZF_ADD(&w.d_freq[bgzf_dist_sym(bdist, &eb, &ev)], 1);
			p += best;
		} else {
			w.tok[p] = 0;
			ARX_BGZF_ADD(&w.ll_freq[in[p]], 1);
			++p;
		}
	}
}
ARX_DEV void bgzf_crc(BgzfWork &w, int n, int lane)
{
	const int s = lane * BGZF_SUB, e = s + BGZF_SUB < n ? s + BGZF_SUB : n;
	uint32_t part = 0;
	if (s < e) {
		uint32_t c = 0xFFFFFFFFu;
		for (int p = s; p < e; ++p) c = w.crc_tab[(c ^ w.in[p]) & 0xFF] ^ (c >> 8);
		c ^= 0xFFFFFFFFu;
		const int last = (n - 1) / BGZF_SUB;
		part = lane == last ? c : bgzf_gf_mul(bgzf_gf_mul(w.xsub[last - 1 - lane], (uint32_t)w.sh[BZ_XTAIL]), c); // behind it: last - 1 - lane whole ranges and the tail
	}
	w.crc_part[lane] = part;
}

// used symbols of freq[0 .. n_sym) by ascending (count, symbol) -> order; the construction counts them itself
ARX_DEV void bgzf_rank(const uint32_t *freq, int n_sym, uint16_t *order, int lane)
{
	for (int s = lane; s < n_sym; s += BGZF_LANES) {
		const uint32_t f = freq[s];
		if (!f) continue;
		int r = 0;
		for (int t = 0; t < n_sym; ++t) { const uint32_t g = freq[t]; r += g && (g < f || (g == f && t < s)); }
		order[r] = (uint16_t)s;
	}
}
// an alphabet with fewer than two used symbols gets its lowest unused ones counted once, as zlib's build_tree does: the code is then always
// complete.  Returns the mask of symbols (0 or 1) that were added; their lengths are not part of the emitted bits' count.
ARX_DEV int bgzf_at_least_two(uint32_t *freq, int n_sym)
{
	int used = 0, mask = 0;
	for (int s = 0; s < n_sym; ++s) used += freq[s] != 0;
	for (int s = 0; s < 2 && used < 2; ++s)
		if (!freq[s]) { freq[s] = 1; mask |= 1 << s; ++used; }
	return mask;
}
// one lane: lengths (at most `limit` bits, Kraft sum exactly 1 for two or more used symbols, 0 for unused symbols) and bit-reversed canonical
// codes.  order: bgzf_rank's; tree: n_sym words; cnt: 64 words.
ARX_DEV void bgzf_build_code(const uint32_t *freq, int n_sym, const uint16_t *order, int limit, uint32_t *A, int32_t *cnt, uint8_t *len, uint16_t *code)
{
	int n = 0;
	for (int s = 0; s < n_sym; ++s) { len[s] = 0; code[s] = 0; n += freq[s] != 0; }
	for (int i = 0; i < 64; ++i) cnt[i] = 0;
	if (n == 0) return;
	if (n == 1) { len[order[0]] = 1; return; }
	for (int i = 0; i < n; ++i) A[i] = freq[order[i]];
	// Moffat & Katajainen, "In-place calculation of minimum-redundancy codes" (1995): parents, then depths of internal nodes, then of leaves
	A[0] += A[1];
	int root = 0, leaf = 2;
	for (int next = 1; next < n - 1; ++next) {
		if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
		if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
	}
	A[n - 2] = 0;
	for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
	int avbl = 1, used = 0, dpth = 0, next = n - 1;
	root = n - 2;
	while (avbl > 0) {
		while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
		while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
		avbl = 2 * used; ++dpth; used = 0;
	}
	for (int i = 0; i < n; ++i) { const int d = (int)A[i]; ++cnt[d < 63 ? d : 63]; } // depth < n, and < 40 for counts that sum to a block's tokens
	// the limit: everything deeper moves up to it, then leaves are moved down (one of the deepest shorter codes becomes two codes one bit longer,
	// a code at the limit takes the freed place) until the Kraft sum, in units of 2^-limit, is 2^limit again
	for (int i = limit + 1; i < 64; ++i) { cnt[limit] += cnt[i]; cnt[i] = 0; }
	uint32_t total = 0;
	for (int i = limit; i > 0; --i) total += (uint32_t)cnt[i] << (limit - i);
	while (total > (1u << limit)) { // at most n rounds: every round takes one unit off
		--cnt[limit];
		for (int i = limit - 1; i > 0; --i)
			if (cnt[i]) { --cnt[i]; cnt[i + 1] += 2; break; }
		--total;
	}
	int j = n;
	for (int i = 1; i <= limit; ++i)
		for (int l = cnt[i]; l > 0; --l) len[order[--j]] = (uint8_t)i; // the most frequent symbols take the shortest codes
	uint32_t nextc[17], c = 0;
	nextc[0] = 0;
	for (int b = 1; b <= limit; ++b) { c = (c + (uint32_t)cnt[b - 1]) << 1; nextc[b] = c; }
	for (int s = 0; s < n_sym; ++s)
		if (len[s]) code[s] = (uint16_t)bgzf_rev(nextc[len[s]]++, len[s]);
}

ARX_DEVI int bgzf_cl_order(int i)
{
	const uint64_t lo = 0x0B050A0609070800ull /* 0,8,7,9,6,10,5,11 */, hi = 0x0F010E020D030C04ull /* 4,12,3,13,2,14,1,15 */;
	return i < 3 ? 16 + i : i < 11 ? (int)((lo >> (8 * (i - 3))) & 0xFF) : (int)((hi >> (8 * (i - 11))) & 0xFF);
}
// one lane, after the two main codes exist: how many lengths the header sends
ARX_DEV void bgzf_header_extent(BgzfWork &w)
{
	int hlit = 286, hdist = 30;
	while (hlit > 257 && !w.ll_len[hlit - 1]) --hlit;
	while (hdist > 1 && !w.d_len[hdist - 1]) --hdist;
	w.sh[BZ_HLIT] = hlit; w.sh[BZ_HDIST] = hdist;
}
ARX_DEV void bgzf_cl_hist(BgzfWork &w, int lane)
{
	const int hlit = w.sh[BZ_HLIT], hdist = w.sh[BZ_HDIST];
	for (int i = lane; i < hlit + hdist; i += BGZF_LANES) ARX_BGZF_ADD(&w.cl_freq[i < hlit ? w.ll_len[i] : w.d_len[i - hlit]], 1);
}
// one lane: the three sizes, the choice
ARX_DEV void bgzf_decide(BgzfWork &w, int n)
{
	int hclen = 19;
	while (hclen > 4 && !w.cl_len[bgzf_cl_order(hclen - 1)]) --hclen;
	w.sh[BZ_HCLEN] = hclen;
	int64_t dyn = 3 + 5 + 5 + 4 + 3 * hclen, fix = 3;
	for (int v = 0; v < BGZF_CL; ++v) dyn += (int64_t)w.cl_freq[v] * w.cl_len[v];
	for (int s = 0; s < 2; ++s)
		if (w.sh[BZ_CL_BUMP] >> s & 1) dyn -= w.cl_len[s];
	for (int s = 0; s < 286; ++s) {
		const int64_t f = w.ll_freq[s];
		dyn += f * (w.ll_len[s] + bgzf_ll_extra(s));
		fix += f * (bgzf_fixed_ll_len(s) + bgzf_ll_extra(s));
	}
	for (int s = 0; s < 30; ++s) {
		const int64_t f = (w.sh[BZ_D_BUMP] >> s & 1) && s < 2 ? 0 : w.d_freq[s];
		dyn += f * (w.d_len[s] + bgzf_d_extra(s));
		fix += f * (5 + bgzf_d_extra(s));
	}
	const int64_t stored_bytes = 5 + n, best = fix <= dyn ? fix : dyn;
	if (stored_bytes <= (best + 7) / 8) { w.sh[BZ_MODE] = BGZF_STORED; w.sh[BZ_BITS] = (int32_t)(8 * stored_bytes); }
	else if (fix <= dyn) { w.sh[BZ_MODE] = BGZF_FIXED; w.sh[BZ_BITS] = (int32_t)fix; }
	else { w.sh[BZ_MODE] = BGZF_DYNAMIC; w.sh[BZ_BITS] = (int32_t)dyn; }
}
// the fixed codes into the code arrays, so that counting and emitting read one form
ARX_DEV void bgzf_fixed_codes(BgzfWork &w, int lane)
{
	if (w.sh[BZ_MODE] != BGZF_FIXED) return;
	for (int s = lane; s < BGZF_LL; s += BGZF_LANES) { const int l = bgzf_fixed_ll_len(s); w.ll_len[s] = (uint8_t)l; w.ll_code[s] = (uint16_t)bgzf_rev(bgzf_fixed_ll_code(s), l); }
	for (int s = lane; s < BGZF_D; s += BGZF_LANES) { w.d_len[s] = 5; w.d_code[s] = (uint16_t)bgzf_rev((uint32_t)s, 5); }
}
ARX_DEVI int bgzf_header_bits(const BgzfWork &w)
{
	if (w.sh[BZ_MODE] != BGZF_DYNAMIC) return 3;
	int b = 17 + 3 * w.sh[BZ_HCLEN];
	for (int i = 0; i < w.sh[BZ_HLIT]; ++i) b += w.cl_len[w.ll_len[i]];
	for (int i = 0; i < w.sh[BZ_HDIST]; ++i) b += w.cl_len[w.d_len[i]];
	return b;
}
ARX_DEV void bgzf_count(BgzfWork &w, int n, int lane)
{
	int b = 0;
	if (w.sh[BZ_MODE] != BGZF_STORED) {
		const int s = lane * BGZF_SUB, e = s + BGZF_SUB < n ? s + BGZF_SUB : n;
		for (int p = s; p < e;) {
			const int t = w.tok[p];
			if (t & 0x8000) {
				int eb, ev;
				const int len = w.tok[p + 1];
				b += w.ll_len[bgzf_len_sym(len, &eb, &ev)] + eb;
				b += w.d_len[bgzf_dist_sym((t & 0x7FFF) + 1, &eb, &ev)] + eb;
				p += len;
			} else { b += w.ll_len[w.in[p]]; ++p; }
		}
		if (lane == 0) b += bgzf_header_bits(w);
		if (lane == BGZF_LANES - 1) b += w.ll_len[256];
	}
	w.bits[lane] = b;
}

struct BgzfBits { // a lane's window on the output: whole words are its own, the first and the last one are shared
	uint32_t *out; uint64_t acc; int nacc, wi; bool first;
	ARX_DEVI void begin(uint32_t *o, int bitpos) { out = o; acc = 0; nacc = bitpos & 31; wi = bitpos >> 5; first = true; }
	ARX_DEVI void put(uint32_t v, int nb) // nb <= 32
	{
		acc |= (uint64_t)v << nacc; nacc += nb;
		if (nacc >= 32) {
			if (first) ARX_BGZF_OR(&out[wi], (uint32_t)acc); else out[wi] = (uint32_t)acc;
			first = false; ++wi; acc >>= 32; nacc -= 32;
		}
	}
	ARX_DEVI void end() { if (nacc > 0 && (uint32_t)acc) ARX_BGZF_OR(&out[wi], (uint32_t)acc); }
};
ARX_DEV void bgzf_zero(BgzfWork &w, uint32_t *out, int lane)
{
	const int words = (w.sh[BZ_BITS] + 31) / 32 + 1; // at most (8 * (5 + 65280) + 31) / 32 + 1 <= BGZF_OUT_SLICE / 4
	for (int i = lane; i < words; i += BGZF_LANES) out[i] = 0;
}
ARX_DEV void bgzf_emit(BgzfWork &w, int n, uint32_t *out, int lane)
{
	if (w.sh[BZ_MODE] == BGZF_STORED) {
		uint8_t *o = (uint8_t *)out;
		if (lane == 0) { o[0] = 1; o[1] = (uint8_t)n; o[2] = (uint8_t)(n >> 8); o[3] = (uint8_t)~n; o[4] = (uint8_t)(~n >> 8); }
		for (int i = lane; i < n; i += BGZF_LANES) o[5 + i] = w.in[i];
		return;
	}
	BgzfBits bw;
	bw.begin(out, w.off[lane]);
	if (lane == 0) {
		if (w.sh[BZ_MODE] == BGZF_FIXED) bw.put(1 | 1 << 1, 3);
		else {
			const int hlit = w.sh[BZ_HLIT], hdist = w.sh[BZ_HDIST], hclen = w.sh[BZ_HCLEN];
			bw.put(1 | 2 << 1, 3);
			bw.put((uint32_t)(hlit - 257), 5); bw.put((uint32_t)(hdist - 1), 5); bw.put((uint32_t)(hclen - 4), 4);
			for (int i = 0; i < hclen; ++i) bw.put(w.cl_len[bgzf_cl_order(i)], 3);
			for (int i = 0; i < hlit; ++i) bw.put(w.cl_code[w.ll_len[i]], w.cl_len[w.ll_len[i]]);
			for (int i = 0; i < hdist; ++i) bw.put(w.cl_code[w.d_len[i]], w.cl_len[w.d_len[i]]);
		}
	}
	const int s = lane * BGZF_SUB, e = s + BGZF_SUB < n ? s + BGZF_SUB : n;
	for (int p = s; p < e;) {
		const int t = w.tok[p];
		if (t & 0x8000) {
			int eb, ev;
			const int len = w.tok[p + 1];
			int sym = bgzf_len_sym(len, &eb, &ev);
			bw.put((uint32_t)w.ll_code[sym] | (uint32_t)ev << w.ll_len[sym], w.ll_len[sym] + eb); // at most 15 + 5 bits
			sym = bgzf_dist_sym((t & 0x7FFF) + 1, &eb, &ev);
			bw.put((uint32_t)w.d_code[sym] | (uint32_t)ev << w.d_len[sym], w.d_len[sym] + eb);   // at most 15 + 13 bits
			p += len;
		} else { bw.put(w.ll_code[w.in[p]], w.ll_len[w.in[p]]); ++p; }
	}
	if (lane == BGZF_LANES - 1) bw.put(w.ll_code[256], w.ll_len[256]);
	bw.end();
}
// one lane: meta[0] bytes of the DEFLATE stream, [1] CRC-32 of the input, [2] the form, [3] input bytes
ARX_DEV void bgzf_finish(BgzfWork &w, int n, uint32_t *meta)
{
	uint32_t crc = 0;
	for (int l = 0; l < BGZF_LANES; ++l) crc ^= w.crc_part[l];
	meta[0] = (uint32_t)((w.sh[BZ_BITS] + 7) / 8); meta[1] = crc; meta[2] = (uint32_t)w.sh[BZ_MODE]; meta[3] = (uint32_t)n;
}

// The block, phase by phase.  drv.lanes(f) runs f(lane) for every lane and ends with a barrier; drv.scan(in, out, n) is an exclusive scan
// (out[n] = total) with the same guarantee.
template <class Drv> ARX_DEV void bgzf_block(Drv &drv, BgzfWork &w, const uint8_t *src, int n, uint32_t *out, uint32_t *meta)
{
	drv.lanes([&](int lane) { bgzf_load(w, src, n, lane); });
	const int chunks = (n + BGZF_CHUNK - 1) / BGZF_CHUNK;
	for (int c = 0; c < chunks; ++c) {
		drv.lanes([&](int lane) { bgzf_cand_read(w, n, c, lane); });
		drv.lanes([&](int lane) { bgzf_cand_insert(w, n, c, lane); });
	}
	drv.lanes([&](int lane) { bgzf_parse(w, n, lane); bgzf_crc(w, n, lane); });
	drv.lanes([&](int lane) { if (lane == 0) w.sh[BZ_D_BUMP] = bgzf_at_least_two(w.d_freq, 30); });
	drv.lanes([&](int lane) { bgzf_rank(w.ll_freq, 286, w.order, lane); bgzf_rank(w.d_freq, 30, w.order + BGZF_LL, lane); });
	drv.lanes([&](int lane) { // the two trees on lanes of different wavefronts
		if (lane == 0) bgzf_build_code(w.ll_freq, 286, w.order, 15, w.tree, w.cnt, w.ll_len, w.ll_code);
		if (lane == BGZF_LANES / 2) bgzf_build_code(w.d_freq, 30, w.order + BGZF_LL, 15, w.tree + BGZF_LL, w.cnt + 64, w.d_len, w.d_code);
	});
	drv.lanes([&](int lane) { if (lane == 0) bgzf_header_extent(w); });
	drv.lanes([&](int lane) { bgzf_cl_hist(w, lane); });
	drv.lanes([&](int lane) { if (lane == 0) w.sh[BZ_CL_BUMP] = bgzf_at_least_two(w.cl_freq, BGZF_CL); });
	drv.lanes([&](int lane) { bgzf_rank(w.cl_freq, BGZF_CL, w.order + 2 * BGZF_LL, lane); });
	drv.lanes([&](int lane) {
		if (lane == 0) {
			bgzf_build_code(w.cl_freq, BGZF_CL, w.order + 2 * BGZF_LL, 7, w.tree + 2 * BGZF_LL, w.cnt + 128, w.cl_len, w.cl_code);
			bgzf_decide(w, n);
		}
	});
	drv.lanes([&](int lane) { bgzf_fixed_codes(w, lane); });
	drv.lanes([&](int lane) { bgzf_count(w, n, lane); bgzf_zero(w, out, lane); });
	drv.scan(w.bits, w.off, BGZF_LANES);
	drv.lanes([&](int lane) { bgzf_emit(w, n, out, lane); if (lane == 0) bgzf_finish(w, n, meta); });
}

} // namespace arx

// dev_inflate.h -- one BGZF block, i.e. one raw DEFLATE stream (RFC 1951) of at most 65536 inflated bytes, back to its bytes plus a status, as
// phases over an explicit lane index: the mirror image of dev_bgzf.h.  hip_inflate.h runs the phases with one wavefront of INF_LANES lanes per
// BGZF block and a wave-scope release/acquire fence where a phase ends; tests/inflatesim/inflate_sim.cpp runs the very same functions on the
// host, lanes in a loop, in either order.  Nothing here knows which of the two it is.
//
// Huffman decoding of one stream is serial, so the parallelism is across the blocks of a launch and, inside a block, in everything except the
// bit-serial decode.  What a stream goes through (inf_block), per DEFLATE block inside it:
//   fill     the wavefront moves the next compressed bytes into a ring of INF_RING bytes in work memory: every byte is read once, with
//            coalesced loads, and only at offsets below the compressed end (what lies behind it reads as zero)
//   header   one lane reads BFINAL and BTYPE; for BTYPE 2 the code lengths through the code length code (a 128-entry table), for BTYPE 1
//            the lanes write the fixed lengths, for BTYPE 0 the lane checks LEN against NLEN
//   setup    one lane counts the lengths, refuses an over-subscribed or incomplete set (the one incomplete set allowed is the distance code
//            with a single 1-bit code; a distance code with no code at all is allowed too: a block without matches) and sorts the symbols
//            by (length, symbol): the canonical order.  One departure from zlib's inflate follows from that rule: a literal/length set
//            of a single 1-bit code (the end-of-block symbol alone), which zlib's inflate accepts and no deflate writes, is
//            INF_BAD_CODE_LENGTHS here
//   tables   the lanes fill the primary tables in parallel, one symbol of the canonical order per lane and round: the entry at every index
//            whose low `length` bits are the symbol's reversed code.  INF_LL_BITS = 10 bits index the literal/length table, INF_D_BITS = 9
//            the distance table.  A longer code (up to 15 bits) finds no entry there and goes through the second level: the canonical
//            walk over the per-length counts and first codes (one compare per bit), which costs 96 bytes where a sub-table per prefix would
//            cost some 9 KB; in a Huffman code a symbol with a code longer than 10 bits is rarer than one in a thousand
//   decode   one lane decodes a batch of at most INF_TOK literals and INF_TOK matches into two lists, from a 64-bit bit buffer refilled a
//            word at a time from the ring.  It keeps the output position as it goes -- it needs it to refuse a distance that reaches before
//            the block's first byte and a byte beyond ISIZE -- so every token is stored with its output offset and no scan is needed
//   literals all lanes write the batch's literals
//   matches  in token order, each as a wave-wide copy, out[o + i] = out[o - dist + (i % dist)]: right for dist < len too.  A fence after each
//            match, because the next one may read what this one wrote
//   stored   BTYPE 0: a wave-wide copy from the compressed bytes
// and behind the stream: the CRC-32 of the produced bytes -- every lane its own range, shifted by x^(8 * bytes behind the range) mod P and
// xor-ed, with dev_bgzf.h's operators -- compared with the trailer's, the size compared with ISIZE, and the bytes copied to their destination.
//
// Where the output lives.  The phases write to `w.out`, whatever memory that is.  The kernel gives it 64 KiB of LDS and copies the finished
// block to its destination in HBM with coalesced stores; it does not decode straight into HBM.  Why: a back-reference reads bytes that other
// lanes wrote one phase earlier, and a block of FASTQ text holds some ten thousand matches, each behind such a hand-off.  Through LDS a
// hand-off costs an LDS round trip; through HBM it costs a store that has to be acknowledged by L2 and a load that goes there again.  By the
// latencies the architecture documents that is several times as long, in a kernel that is bound by exactly this latency; it is an
// estimate: no variant that decodes into HBM was built or measured.  The price is occupancy: 78 KB of LDS a wavefront, two wavefronts a
// CU.  A launch of the feeder holds a few hundred blocks and the MI355X has 256 CUs, so the expectation (again not measured) is that
// the limit is seldom reached.
//
// Safety is structural: every read of compressed bytes is at an offset below `clen`, every write at an offset below `isize` <= INF_MAX_OUT,
// every table index is masked or compared with the table's size, every list index with INF_TOK, and every loop ends by a count derived
// from one of these.  A damaged stream gives a status, never an access out of range.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "bgzf_walk.h" // InfRow, INF_MAX_OUT, and the host's walk over the block headers
#include "dev_bgzf.h" // the CRC-32 operators (BGZF_POLY, bgzf_gf_mul, bgzf_x8n), bgzf_rev, bgzf_cl_order, bgzf_fixed_ll_len

namespace arx {

constexpr int INF_LANES = 64;       // one wavefront
constexpr int INF_MAX_IN = 65536;   // ... and compressed (BSIZE is 16 bits)
constexpr int INF_LL_BITS = 10, INF_D_BITS = 9, INF_CL_BITS = 7;
constexpr int INF_RING = 4096;      // bytes of the compressed stream in work memory (a power of two)
constexpr int INF_PAD = 16;         // bytes behind the compressed end that read as zero; a token takes at most 48 bits, a refill 4 bytes
constexpr int INF_TOK = 256;        // literals, and matches, of a batch: at most 2 * 256 * 6 bytes of the ring
constexpr int INF_LL = 288, INF_D = 32; // alphabet sizes as the fixed code has them (286 and 30 symbols are valid)
enum { INF_OK = 0, INF_BAD_HEADER, INF_BAD_BTYPE, INF_BAD_STORED_LEN, INF_BAD_CODE_LENGTHS, INF_BAD_SYMBOL, INF_BAD_DISTANCE, INF_TRUNCATED, INF_SIZE_MISMATCH,
       INF_CRC_MISMATCH, INF_N_STATUS };
// shared scalars of a stream
enum { IS_BITPOS = 0, IS_OUTPOS, IS_STATUS, IS_FINAL, IS_BTYPE, IS_NDEFL, IS_HI, IS_ST_SRC, IS_ST_DST, IS_ST_LEN, IS_NLIT, IS_NM, IS_EOB, IS_NSYM_LL, IS_NSYM_D, IS_BASE, IS_N_SCALARS };
static_assert((INF_RING & (INF_RING - 1)) == 0 && INF_RING >= 2 * INF_TOK * 6 + INF_PAD + 600, "the ring holds a batch, and a dynamic header (at most 563 bytes)");

struct InfWork {
	uint8_t *out;        // INF_MAX_OUT: the block's bytes
	uint8_t *ring;       // INF_RING, 4-aligned: byte i of the stream at i & (INF_RING - 1)
	uint16_t *ll_tab, *d_tab; // primary tables: symbol << 4 | length, 0: no code of at most that many bits
	uint8_t *cl_tab;     // the code length code: symbol << 3 | length
	uint8_t *len;        // INF_LL + INF_D code lengths
	uint8_t *cl_len;     // 19 (+ 1)
	uint16_t *sym;       // INF_LL + INF_D: the symbols in canonical order
	int32_t *cnt, *first, *index; // 2 x 16 each: codes per length, the first code of a length, where its symbols start in sym
	uint16_t *lit_off; uint8_t *lit_val;       // INF_TOK: the batch's literals
	uint16_t *m_off, *m_len, *m_dist;          // INF_TOK: ... and matches
	uint32_t *crc_tab, *x2n, *crc_part;        // 256, 32, INF_LANES
	int32_t *sh;         // IS_N_SCALARS
};
constexpr int INF_WORK_BYTES = INF_RING + 2 * (1 << INF_LL_BITS) + 2 * (1 << INF_D_BITS) + 2 * (INF_LL + INF_D) + 3 * 4 * 32 + 2 * INF_TOK + 3 * 2 * INF_TOK +
                               4 * (256 + 32 + INF_LANES) + 4 * IS_N_SCALARS + (INF_LL + INF_D) + INF_TOK + 20 + (1 << INF_CL_BITS);

// carves the arrays out of one 4-aligned buffer of INF_WORK_BYTES bytes; `out` is given apart (INF_MAX_OUT bytes)
ARX_DEVI void inf_carve(InfWork &w, uint8_t *mem, uint8_t *out)
{
	uint8_t *p = mem;
	w.out = out;
	w.ring = p; p += INF_RING;
	w.cnt = (int32_t *)p; p += 4 * 32;
	w.first = (int32_t *)p; p += 4 * 32;
	w.index = (int32_t *)p; p += 4 * 32;
	w.crc_tab = (uint32_t *)p; p += 4 * 256;
	w.x2n = (uint32_t *)p; p += 4 * 32;
	w.crc_part = (uint32_t *)p; p += 4 * INF_LANES;
	w.sh = (int32_t *)p; p += 4 * IS_N_SCALARS;
	w.ll_tab = (uint16_t *)p; p += 2 * (1 << INF_LL_BITS);
	w.d_tab = (uint16_t *)p; p += 2 * (1 << INF_D_BITS);
	w.sym = (uint16_t *)p; p += 2 * (INF_LL + INF_D);
	w.lit_off = (uint16_t *)p; p += 2 * INF_TOK;
	w.m_off = (uint16_t *)p; p += 2 * INF_TOK;
	w.m_len = (uint16_t *)p; p += 2 * INF_TOK;
	w.m_dist = (uint16_t *)p; p += 2 * INF_TOK;
	w.len = p; p += INF_LL + INF_D;
	w.lit_val = p; p += INF_TOK;
	w.cl_len = p; p += 20;
	w.cl_tab = p; p += 1 << INF_CL_BITS;
}

// ---- the bit reader of the one decoding lane: a 64-bit buffer over the ring's words.  After refill() it holds at least 33 bits
struct InfBits {
	const uint32_t *ring; uint64_t buf; int n, wpos;
	ARX_DEVI void begin(const uint8_t *r, int bitpos)
	{
		ring = (const uint32_t *)r; wpos = bitpos >> 5;
		buf = (uint64_t)ring[wpos & (INF_RING / 4 - 1)] >> (bitpos & 31); n = 32 - (bitpos & 31); ++wpos;
		refill();
	}
	ARX_DEVI void refill() { if (n <= 32) { buf |= (uint64_t)ring[wpos & (INF_RING / 4 - 1)] << n; n += 32; ++wpos; } }
	ARX_DEVI uint32_t peek(int k) const { return (uint32_t)buf & ((1u << k) - 1u); } // k <= 16
	ARX_DEVI void drop(int k) { buf >>= k; n -= k; }
	ARX_DEVI uint32_t get(int k) { const uint32_t v = peek(k); drop(k); return v; }
	ARX_DEVI int pos() const { return wpos * 32 - n; }
};
// the end of what the ring holds once it was filled for a stream position
ARX_DEVI int inf_ring_hi(int bitpos, int clen)
{
	const int lo = (bitpos >> 3) & ~3, end = (clen + INF_PAD + 3) & ~3;
	return lo + INF_RING < end ? lo + INF_RING : end;
}

// ---- phases.  src[0, clen): the stream; the block inflates to `isize` bytes
ARX_DEV void inf_begin(InfWork &w, int lane)
{
	for (int i = lane; i < 256; i += INF_LANES) {
		uint32_t c = (uint32_t)i;
		for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ BGZF_POLY : c >> 1;
		w.crc_tab[i] = c;
	}
	if (lane == 0) {
		uint32_t p = 0x40000000u; // x^1
		w.x2n[0] = p;
		for (int k = 1; k < 32; ++k) { p = bgzf_gf_mul(p, p); w.x2n[k] = p; }
		for (int i = 0; i < IS_N_SCALARS; ++i) w.sh[i] = 0;
	}
}
ARX_DEV void inf_fill(InfWork &w, const uint8_t *src, int clen, int lane)
{
	const int lo = (w.sh[IS_BITPOS] >> 3) & ~3, hi = inf_ring_hi(w.sh[IS_BITPOS], clen);
	const int from = w.sh[IS_HI] > lo ? w.sh[IS_HI] : lo; // what is there already stays; IS_HI is moved by the next one-lane phase
	for (int i = from + lane; i < hi; i += INF_LANES) w.ring[i & (INF_RING - 1)] = i < clen ? src[i] : (uint8_t)0;
}

// one lane: lengths `len[0, n)` -> counts, first codes, canonical order; INF_OK or INF_BAD_CODE_LENGTHS.  single_ok: the distance code's rules
ARX_DEV int inf_code_setup(const uint8_t *len, int n, int32_t *cnt, int32_t *first, int32_t *index, uint16_t *sym, bool single_ok, int32_t *n_used)
{
	for (int l = 0; l < 16; ++l) cnt[l] = 0;
	for (int s = 0; s < n; ++s) ++cnt[len[s] & 15];
	int left = 1, used = 0;
	for (int l = 1; l < 16; ++l) {
		left = (left << 1) - cnt[l];
		if (left < 0) return INF_BAD_CODE_LENGTHS; // over-subscribed
		used += cnt[l];
	}
	if (left > 0 && !(single_ok && (used == 0 || (used == 1 && cnt[1] == 1)))) return INF_BAD_CODE_LENGTHS; // incomplete
	int code = 0, at = 0;
	for (int l = 1; l < 16; ++l) { first[l] = code; index[l] = at; at += cnt[l]; code = (code + cnt[l]) << 1; }
	first[0] = 0; index[0] = 0;
	// cnt[l] is consumed as the running fill of length l and restored below
	for (int l = 1; l < 16; ++l) cnt[l] = 0;
	for (int s = 0; s < n; ++s) {
		const int l = len[s] & 15;
		if (l) { sym[index[l] + cnt[l]] = (uint16_t)s; ++cnt[l]; }
	}
	*n_used = used;
	return INF_OK;
}
// all lanes: the primary table of 1 << bits entries, cleared
ARX_DEV void inf_table_clear(uint16_t *tab, int bits, int lane)
{
	for (int i = lane; i < (1 << bits); i += INF_LANES) tab[i] = 0;
}
// all lanes: symbol i of the canonical order into every entry its code is a prefix of
ARX_DEV void inf_table_fill(uint16_t *tab, int bits, const uint8_t *len, const int32_t *first, const int32_t *index, const uint16_t *sym, int n_used, int lane)
{
	for (int i = lane; i < n_used; i += INF_LANES) {
		const int s = sym[i], l = len[s] & 15;
		if (l == 0 || l > bits) continue;
		const uint32_t code = (uint32_t)(first[l] + (i - index[l]));
		for (uint32_t k = bgzf_rev(code, l); k < (1u << bits); k += 1u << l) tab[k] = (uint16_t)(s << 4 | l);
	}
}
// one symbol: the primary table, or the walk over the lengths; -1: no such code.  The reader holds at least 15 bits
ARX_DEVI int inf_symbol(InfBits &b, const uint16_t *tab, int bits, const int32_t *cnt, const int32_t *first, const int32_t *index, const uint16_t *sym, int n_sym)
{
	const uint32_t e = tab[b.peek(bits)];
	if (e & 15) { b.drop((int)(e & 15)); return (int)(e >> 4); }
	int code = 0;
	for (int l = 1; l < 16; ++l) {
		code = code << 1 | (int)((b.buf >> (l - 1)) & 1);
		const int d = code - first[l];
		if (d >= 0 && d < cnt[l]) {
			const int at = index[l] + d;
			b.drop(l);
			return at < n_sym ? (int)sym[at] : -1;
		}
	}
	return -1;
}

// one lane: the header of the next DEFLATE block
ARX_DEV void inf_header(InfWork &w, int clen, int isize)
{
	int32_t *sh = w.sh;
	sh[IS_HI] = inf_ring_hi(sh[IS_BITPOS], clen);
	InfBits b;
	b.begin(w.ring, sh[IS_BITPOS]);
	if (b.pos() + 3 > 8 * clen) { sh[IS_STATUS] = INF_TRUNCATED; return; }
	sh[IS_FINAL] = (int32_t)b.get(1);
	const int type = (int)b.get(2);
	sh[IS_BTYPE] = type; ++sh[IS_NDEFL];
	if (type == 3) { sh[IS_STATUS] = INF_BAD_BTYPE; return; }
	if (type == 0) {
		const int at = (b.pos() + 7) >> 3; // LEN and NLEN start at the next byte
		if (at + 4 > clen) { sh[IS_STATUS] = INF_TRUNCATED; return; }
		const uint8_t *r = w.ring;
		const int n = r[at & (INF_RING - 1)] | r[(at + 1) & (INF_RING - 1)] << 8, nn = r[(at + 2) & (INF_RING - 1)] | r[(at + 3) & (INF_RING - 1)] << 8;
		if ((n ^ 0xFFFF) != nn) { sh[IS_STATUS] = INF_BAD_STORED_LEN; return; }
		if (at + 4 + n > clen) { sh[IS_STATUS] = INF_TRUNCATED; return; }
		if (sh[IS_OUTPOS] + n > isize) { sh[IS_STATUS] = INF_SIZE_MISMATCH; return; }
		sh[IS_ST_SRC] = at + 4; sh[IS_ST_DST] = sh[IS_OUTPOS]; sh[IS_ST_LEN] = n;
		sh[IS_OUTPOS] += n; sh[IS_BITPOS] = 8 * (at + 4 + n);
		return;
	}
	if (type == 1) { sh[IS_BITPOS] = b.pos(); return; } // the lengths are written by all lanes (inf_fixed_lengths)
	const int hlit = (int)b.get(5) + 257, hdist = (int)b.get(5) + 1, hclen = (int)b.get(4) + 4;
	if (hlit > 286 || hdist > 30) { sh[IS_STATUS] = INF_BAD_CODE_LENGTHS; return; }
	for (int i = 0; i < 19; ++i) w.cl_len[i] = 0;
	for (int i = 0; i < hclen; ++i) { b.refill(); w.cl_len[bgzf_cl_order(i)] = (uint8_t)b.get(3); }
	if (b.pos() > 8 * clen) { sh[IS_STATUS] = INF_TRUNCATED; return; }
	// the code length code: complete, 7 bits at most -> a full table, filled by this lane (19 symbols)
	int32_t *cnt = w.cnt, *first = w.first, *index = w.index, used = 0;
	if (inf_code_setup(w.cl_len, 19, cnt, first, index, w.sym, false, &used) != INF_OK) { sh[IS_STATUS] = INF_BAD_CODE_LENGTHS; return; }
	for (int i = 0; i < used && i < 19; ++i) {
		const int s = w.sym[i], l = w.cl_len[s] & 7;
		if (l == 0) continue;
		const uint32_t code = (uint32_t)(first[l] + (i - index[l]));
		for (uint32_t k = bgzf_rev(code, l); k < (1u << INF_CL_BITS); k += 1u << l) w.cl_tab[k] = (uint8_t)(s << 3 | l);
	}
	const int n = hlit + hdist;
	int prev = 0;
	for (int i = 0; i < n;) { // every round writes at least one length
		b.refill();
		const uint32_t e = w.cl_tab[b.peek(INF_CL_BITS)];
		const int s = (int)(e >> 3);
		b.drop((int)(e & 7));
		int rep = 1, val = s;
		if (s == 16) { rep = 3 + (int)b.get(2); val = prev; }
		else if (s == 17) { rep = 3 + (int)b.get(3); val = 0; }
		else if (s == 18) { rep = 11 + (int)b.get(7); val = 0; }
		if (b.pos() > 8 * clen) { sh[IS_STATUS] = INF_TRUNCATED; return; }
		if ((s == 16 && i == 0) || i + rep > n) { sh[IS_STATUS] = INF_BAD_CODE_LENGTHS; return; }
		for (int k = 0; k < rep; ++k, ++i) w.len[i < hlit ? i : INF_LL + (i - hlit)] = (uint8_t)val;
		prev = val;
	}
	for (int i = hlit; i < INF_LL; ++i) w.len[i] = 0;
	for (int i = hdist; i < INF_D; ++i) w.len[INF_LL + i] = 0;
	sh[IS_BITPOS] = b.pos();
}
ARX_DEV void inf_fixed_lengths(InfWork &w, int lane)
{
	for (int s = lane; s < INF_LL; s += INF_LANES) w.len[s] = (uint8_t)bgzf_fixed_ll_len(s);
	for (int s = lane; s < INF_D; s += INF_LANES) w.len[INF_LL + s] = 5;
}
// one lane: both codes of a block with BTYPE 1 or 2
ARX_DEV void inf_codes(InfWork &w)
{
	int32_t *sh = w.sh;
	if (w.len[256] == 0) { sh[IS_STATUS] = INF_BAD_CODE_LENGTHS; return; } // no end of block
	if (inf_code_setup(w.len, INF_LL, w.cnt, w.first, w.index, w.sym, false, &sh[IS_NSYM_LL]) != INF_OK ||
	    inf_code_setup(w.len + INF_LL, INF_D, w.cnt + 16, w.first + 16, w.index + 16, w.sym + INF_LL, true, &sh[IS_NSYM_D]) != INF_OK)
		sh[IS_STATUS] = INF_BAD_CODE_LENGTHS;
}
ARX_DEV void inf_stored(InfWork &w, const uint8_t *src, int lane)
{
	const int s = w.sh[IS_ST_SRC], d = w.sh[IS_ST_DST], n = w.sh[IS_ST_LEN]; // s + n <= clen and d + n <= isize (inf_header)
	for (int i = lane; i < n; i += INF_LANES) w.out[d + i] = src[s + i];
}

// one lane: the next batch of tokens.  WINDOWED (dev_gunzip.h): the stream goes on from a place whose 32 KiB of history lie outside `out`, so a
// distance may reach up to 32768 bytes before the first one; the offsets of the batch's tokens count from the output position the batch began
// at (IS_BASE), and the batch ends before its output could span more than `span` bytes.  Otherwise (a BGZF block) they count from 0
template <bool WINDOWED> ARX_DEV void inf_decode_t(InfWork &w, int clen, int isize, int span)
{
	int32_t *sh = w.sh;
	const int hi = inf_ring_hi(sh[IS_BITPOS], clen);
	const bool more = hi < ((clen + INF_PAD + 3) & ~3);
	sh[IS_HI] = hi;
	InfBits b;
	b.begin(w.ring, sh[IS_BITPOS]);
	int o = sh[IS_OUTPOS], nl = 0, nm = 0, eob = 0, st = INF_OK;
	const int base = WINDOWED ? o : 0;
	sh[IS_BASE] = base;
	while (nl < INF_TOK && nm < INF_TOK) { // every round takes at least one bit or ends the loop
		if (WINDOWED && o - base + 258 > span) break; // (a token is at most 258 bytes)
		const int pos = b.pos();
		if (pos > 8 * clen) { st = INF_TRUNCATED; break; }
		if (more && (pos >> 3) + INF_PAD > hi) break; // the ring is refilled first
		b.refill();
		const int s = inf_symbol(b, w.ll_tab, INF_LL_BITS, w.cnt, w.first, w.index, w.sym, INF_LL);
		// a symbol read from bits behind the end is the end's fault; so is no symbol in 15 bits that are not all there
		if (b.pos() > 8 * clen || (s < 0 && b.pos() + 15 > 8 * clen)) { st = INF_TRUNCATED; break; }
		if (s < 0 || s >= 286) { st = INF_BAD_SYMBOL; break; }
		if (s < 256) {
			if (o >= isize) { st = INF_SIZE_MISMATCH; break; }
			w.lit_off[nl] = (uint16_t)(o - base); w.lit_val[nl] = (uint8_t)s; ++nl; ++o;
			continue;
		}
		if (s == 256) { eob = 1; break; }
		int len;
		if (s == 285) len = 258;
		else {
			const int l = s - 257;
			if (l < 8) len = 3 + l;
			else { const int e = (l >> 2) - 1; len = 3 + ((4 + (l & 3)) << e) + (int)b.get(e); }
		}
		b.refill();
		const int ds = inf_symbol(b, w.d_tab, INF_D_BITS, w.cnt + 16, w.first + 16, w.index + 16, w.sym + INF_LL, INF_D);
		if (b.pos() > 8 * clen || (ds < 0 && b.pos() + 15 > 8 * clen)) { st = INF_TRUNCATED; break; }
		if (ds < 0 || ds >= 30) { st = INF_BAD_SYMBOL; break; }
		int dist;
		if (ds < 4) dist = ds + 1;
		else { const int e = (ds >> 1) - 1; dist = 1 + ((2 + (ds & 1)) << e) + (int)b.get(e); }
		if (b.pos() > 8 * clen) { st = INF_TRUNCATED; break; }
		if (!WINDOWED && dist > o) { st = INF_BAD_DISTANCE; break; }
		if (o + len > isize) { st = INF_SIZE_MISMATCH; break; }
		w.m_off[nm] = (uint16_t)(o - base); w.m_len[nm] = (uint16_t)len; w.m_dist[nm] = (uint16_t)(dist - 1); ++nm;
		o += len;
	}
	if (st == INF_OK && b.pos() > 8 * clen) st = INF_TRUNCATED;
	sh[IS_STATUS] = st;
	sh[IS_NLIT] = st == INF_OK ? nl : 0; sh[IS_NM] = st == INF_OK ? nm : 0; sh[IS_EOB] = eob;
	sh[IS_OUTPOS] = o; sh[IS_BITPOS] = b.pos();
}
ARX_DEV void inf_decode(InfWork &w, int clen, int isize) { inf_decode_t<false>(w, clen, isize, 0); }
ARX_DEV void inf_literals(InfWork &w, int lane)
{
	const int n = w.sh[IS_NLIT];
	for (int i = lane; i < n && i < INF_TOK; i += INF_LANES) w.out[w.lit_off[i]] = w.lit_val[i];
}
ARX_DEV void inf_match(InfWork &w, int k, int lane) // k < IS_NM <= INF_TOK; dist <= o and o + len <= isize (inf_decode)
{
	const int o = w.m_off[k], len = w.m_len[k], dist = w.m_dist[k] + 1;
	const uint8_t *from = w.out + (o - dist);
	for (int i = lane; i < len; i += INF_LANES) w.out[o + i] = from[dist >= len ? i : i % dist];
}

// what the bytes byte(s) .. byte(e - 1) of an n-byte message add to its CRC-32: their own CRC shifted by x^(8 * bytes behind them) mod P.  The
// xor of these over ranges that tile [0, n) is the message's CRC
template <class Byte> ARX_DEVI uint32_t inf_crc_range(const uint32_t *crc_tab, const uint32_t *x2n, Byte byte, int64_t s, int64_t e, int64_t n)
{
	if (s >= e) return 0;
	uint32_t c = 0xFFFFFFFFu;
	for (int64_t p = s; p < e; ++p) c = crc_tab[(c ^ byte(p)) & 0xFF] ^ (c >> 8);
	c ^= 0xFFFFFFFFu;
	return e < n ? bgzf_gf_mul(bgzf_x8n(x2n, (uint32_t)(n - e)), c) : c;
}
ARX_DEV void inf_crc(InfWork &w, int n, int lane)
{
	const int per = (n + INF_LANES - 1) / INF_LANES, s = lane * per < n ? lane * per : n, e = s + per < n ? s + per : n;
	w.crc_part[lane] = inf_crc_range(w.crc_tab, w.x2n, [&](int64_t p) { return w.out[p]; }, s, e, n);
}
// one lane: the block's status
ARX_DEV void inf_finish(InfWork &w, int isize, uint32_t want_crc)
{
	int st = w.sh[IS_STATUS];
	if (st == INF_OK && w.sh[IS_OUTPOS] != isize) st = INF_SIZE_MISMATCH;
	uint32_t crc = 0;
	for (int l = 0; l < INF_LANES; ++l) crc ^= w.crc_part[l];
	if (st == INF_OK && crc != want_crc) st = INF_CRC_MISMATCH;
	w.sh[IS_STATUS] = st;
}
// all lanes: the finished block to its destination; whole words where both sides are aligned alike
ARX_DEV void inf_copy_out(const uint8_t *from, uint8_t *dst, int n, int lane)
{
	if ((((uintptr_t)from ^ (uintptr_t)dst) & 3) == 0) {
		int head = (int)((4 - ((uintptr_t)dst & 3)) & 3);
		if (head > n) head = n;
		const int words = (n - head) >> 2;
		if (lane < head) dst[lane] = from[lane];
		const uint32_t *s4 = (const uint32_t *)(from + head);
		uint32_t *d4 = (uint32_t *)(dst + head);
		for (int i = lane; i < words; i += INF_LANES) d4[i] = s4[i];
		for (int i = head + 4 * words + lane; i < n; i += INF_LANES) dst[i] = from[i];
	} else
		for (int i = lane; i < n; i += INF_LANES) dst[i] = from[i];
}

// a row that stays inside the launch's compressed bytes and output
ARX_DEVI bool inf_row_in_range(const InfRow &r, int64_t src_bytes, int64_t out_bytes)
{
	return r.clen >= 0 && r.isize >= 0 && r.coff >= 0 && r.ooff >= 0 && r.clen <= src_bytes && r.coff <= src_bytes - r.clen && r.isize <= out_bytes && r.ooff <= out_bytes - r.isize;
}

// The stream, phase by phase.  drv.lanes(f) runs f(lane) for every lane and ends with the hand-off (on the GPU: a wave-scope release, the
// wave barrier, a wave-scope acquire); what a phase reads of the shared scalars was written in an earlier phase, so the control flow is the
// same on every lane.  Returns the status; *n_deflate: DEFLATE blocks whose header was read.  dst receives the bytes of a block that is INF_OK
template <class Drv> ARX_DEV int inf_block(Drv &drv, InfWork &w, const uint8_t *src, int clen, int isize, uint32_t want_crc, uint8_t *dst, int *n_deflate)
{
	*n_deflate = 0;
	if (clen < 0 || clen > INF_MAX_IN || isize < 0 || isize > INF_MAX_OUT) return INF_BAD_HEADER;
	drv.lanes([&](int lane) { inf_begin(w, lane); });
	int32_t *sh = w.sh;
	// a DEFLATE block takes at least 3 bits, a batch at least one: both loops end by the stream's length even before the checks inside do
	for (int blocks = 0; blocks <= 8 * clen && sh[IS_STATUS] == INF_OK; ++blocks) {
		drv.lanes([&](int lane) { inf_fill(w, src, clen, lane); });
		drv.lanes([&](int lane) { if (lane == 0) inf_header(w, clen, isize); });
		if (sh[IS_STATUS] != INF_OK) break;
		if (sh[IS_BTYPE] == 0) drv.lanes([&](int lane) { inf_stored(w, src, lane); });
		else {
			if (sh[IS_BTYPE] == 1) drv.lanes([&](int lane) { inf_fixed_lengths(w, lane); });
			drv.lanes([&](int lane) {
				if (lane == 0) inf_codes(w);
				inf_table_clear(w.ll_tab, INF_LL_BITS, lane); inf_table_clear(w.d_tab, INF_D_BITS, lane);
			});
			if (sh[IS_STATUS] != INF_OK) break;
			drv.lanes([&](int lane) {
				inf_table_fill(w.ll_tab, INF_LL_BITS, w.len, w.first, w.index, w.sym, sh[IS_NSYM_LL], lane);
				inf_table_fill(w.d_tab, INF_D_BITS, w.len + INF_LL, w.first + 16, w.index + 16, w.sym + INF_LL, sh[IS_NSYM_D], lane);
			});
			for (int batches = 0; batches <= 8 * clen; ++batches) {
				drv.lanes([&](int lane) { inf_fill(w, src, clen, lane); });
				drv.lanes([&](int lane) { if (lane == 0) inf_decode(w, clen, isize); });
				if (sh[IS_STATUS] != INF_OK) break;
				drv.lanes([&](int lane) { inf_literals(w, lane); });
				const int nm = sh[IS_NM] < INF_TOK ? sh[IS_NM] : INF_TOK;
				for (int k = 0; k < nm; ++k) drv.lanes([&](int lane) { inf_match(w, k, lane); });
				if (sh[IS_EOB]) break;
			}
		}
		if (sh[IS_FINAL]) break;
	}
	const int n = sh[IS_STATUS] != INF_OK ? 0 : sh[IS_OUTPOS] < isize ? sh[IS_OUTPOS] : isize;
	drv.lanes([&](int lane) { inf_crc(w, n, lane); });
	drv.lanes([&](int lane) { if (lane == 0) inf_finish(w, isize, want_crc); });
	const int st = sh[IS_STATUS];
	*n_deflate = sh[IS_NDEFL];
	if (st == INF_OK) drv.lanes([&](int lane) { inf_copy_out(w.out, dst, isize, lane); });
	return st;
}

} // namespace arx

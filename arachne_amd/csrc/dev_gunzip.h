// dev_gunzip.h -- one plain DEFLATE stream (a gzip member's body: no BGZF framing) inflated by many wavefronts at once, as phases over an
// explicit lane index, in the manner of dev_inflate.h, whose header, code, table and symbol functions it runs.  hip_gunzip.h runs the phases on
// the GPU; tests/gunzipsim/gunzip_sim.cpp runs the very same functions on the host, lanes in a loop, in either order.  Nothing here knows which
// of the two it is.  The scheme is the two-pass one of pugz and rapidgzip.
//
// A launch is given the compressed bytes of a slab, src[0, clen), the bit at which a DEFLATE block is known to start (start_bit: the member's
// first block, or where the launch before ended), and the 32 KiB of text in front of that point with the number of them that exist (the
// carried window).  Chunk k owns the bits [8 k chunk_bytes, 8 (k + 1) chunk_bytes) of the slab.
//   find     (gz_find, a wavefront per chunk) chunk 0 starts at start_bit.  Every other chunk looks for the first bit of its range at which a
//            non-final dynamic block may start: the lanes test 64 consecutive positions against the cheap fields (BFINAL = 0, BTYPE = 2,
//            HLIT <= 286, HDIST <= 30, a code length code whose Kraft sum is exactly one), and what survives is checked whole, one position
//            at a time, by inf_header and inf_codes.  A chunk without such a position has no candidate and decodes nothing
//   decode   (gz_decode, a wavefront per chunk with a candidate) DEFLATE blocks of all three types from the candidate to the first block
//            boundary at or behind the next chunk's candidate; the last such chunk runs until the bytes end and keeps what its last completed
//            block left.  The output is 16-bit symbols: a value below 256 is a byte, 256 + i is byte i of the 32 KiB in front of the chunk's
//            first output byte (a marker).  A match copies symbols, so markers propagate by themselves.  Every symbol goes to the chunk's span
//            of a staging buffer (write-only) and to a ring in work memory that serves the back-references
//   chain    (gz_chain, one lane) the accepted chain: chunk 0 and every following chunk whose predecessor was accepted and ended exactly on
//            its candidate.  It stops at a chunk that is not GZ_OK, behind one that ended a member, and behind one that did not end on the next
//            candidate (it passed it: the candidate was false; or the bytes ended first)
//   windows  (gz_window_at) W[m + 1] = the last 32 KiB of (W[m] followed by the m-th accepted chunk's symbols, markers replaced through W[m]);
//            W[0] is the carried window.  Sequential over the chain, parallel over the 32 Ki entries.  Every W is kept.  Where W[m] is not
//            full (the first 32 KiB of a member) the chunk's markers are checked on the way (gz_bad_marker_at): one that names a byte the
//            window does not have -- the stream reaches in front of its member's start -- is counted, and the host hands such a stream to zlib
// Now the sizes are known: the host says where the text goes, and
//   resolve  (gz_resolve_at, gz_crc_part) all accepted chunks at once: text[off + i] = sym < 256 ? sym : W[m][sym - 256], written at its final
//            place, and the CRC-32 of each chunk's bytes with dev_bgzf.h's operators
// The device never declares a stream bad: whatever it does not take is reported, and the host's zlib decides (gunzip_host.h).
//
// The ring.  The literals of a batch are written before its matches, so a late literal of a batch could overwrite a ring slot that an earlier
// match of the same batch still has to read.  A write at output position q lands on the slot of q - GZ_RING; a match at o >= base reads no
// position below base - 32768.  With the batch's output span capped at GZ_SPAN (inf_decode_t<true>) q < base + GZ_SPAN, so
// q - GZ_RING < base - 32768 exactly when GZ_RING >= 32768 + GZ_SPAN: the hazard is excluded by construction (the static_assert below).
// Of the two sizes that do this, 65,536 entries with a span of 32,768 is 128 KiB plus the tables: one wavefront a CU.  32,768 + 1,536 entries
// is 67 KiB plus the tables, just under half of the 160 KiB of a CU: two wavefronts a CU, and a batch of at most 256 + 256 tokens of FASTQ text
// seldom spans 1,536 bytes, so the cap rarely ends a batch early.  The second was built; neither was measured against the other.
//
// Safety is structural, as in dev_inflate.h: reads of compressed bytes lie below clen, staging writes below the chunk's capacity (inf_header
// and inf_decode_t compare the output position with it), ring indices are taken modulo GZ_RING, window indices are below 32768 by the symbol's
// range, and every loop ends by a count.
#pragma once
#include "dev_inflate.h"

namespace arx {

constexpr int GZ_WIN = 32768;             // DEFLATE's history
constexpr int GZ_SPAN = 1536;             // symbols a batch may span
constexpr int GZ_RING = 34304;            // entries of the ring: symbol p at p % GZ_RING
constexpr int GZ_PIECE = 2048;            // bytes whose bit positions are searched per fill of the compressed ring
constexpr int64_t GZ_MAX_SLAB = 1 << 27;  // bit positions are 32-bit
constexpr int64_t GZ_MAX_CHUNKS = 1 << 14; // chunks of a launch: a window of 32 KiB is kept per chunk (512 MiB at the most)
constexpr int64_t GZ_MAX_SYMBOLS = 1 << 30; // ... and so are a chunk's output positions
static_assert(GZ_RING >= GZ_WIN + GZ_SPAN, "a literal of a batch never lands on a slot a match of the same batch reads");
static_assert(GZ_SPAN >= 2 * 258 && GZ_SPAN <= 65535, "a batch holds a token, and its offsets are 16 bits");
static_assert(GZ_PIECE + 128 <= INF_RING, "the cheap check reads 74 bits behind the last position of a piece");

enum { GZ_OK = 0, GZ_NO_CANDIDATE, GZ_OVERFLOW, GZ_NO_BLOCK, GZ_BAD_STREAM };         // GzChunk::status
enum { GZ_F_CONFIRMED = 1, GZ_F_PASSED = 2, GZ_F_MEMBER_END = 4, GZ_F_ACCEPTED = 8 }; // GzChunk::flags
struct GzChunk {
	int32_t cand;    // the bit its decode starts at; -1: none
	int32_t next;    // the next chunk with a candidate; n_chunks: none
	int32_t end_bit; // where its last completed block ended
	int32_t count;   // symbols produced up to there
	int32_t status;  // GZ_*
	int32_t inf;     // dev_inflate.h's status where that is GZ_BAD_STREAM
	int32_t flags;   // GZ_F_*
	int32_t blocks;  // DEFLATE blocks completed
	int32_t order;   // accepted: its place in the chain, which is the window in front of it
	int32_t bad_markers; // markers that name a byte the window does not have
	uint32_t crc;    // of its bytes
	int32_t markers; // markers replaced
	int32_t have, pad; // accepted: bytes that exist of the window in front of it
	int64_t stage_off, stage_cap; // its span of the staging buffer
	int64_t text_off; // accepted: where its bytes go
};
struct GzChain { int32_t n_accepted, last, have; int32_t pad; int64_t text_bytes; }; // last: the last accepted chunk; have: bytes of the final window that exist

struct GzWork {
	InfWork inf;
	uint16_t *ring; // GZ_RING
	uint8_t *surv;  // INF_LANES: the positions of a round that pass the cheap check
	int32_t *gs;    // GS_N
};
enum { GS_PICK = 0, GS_N = 4 };
constexpr int GZ_FIND_BYTES = ((INF_WORK_BYTES + 15) & ~15) + 4 * GS_N + INF_LANES, GZ_WORK_BYTES = GZ_FIND_BYTES + 2 * GZ_RING;
static_assert(GZ_FIND_BYTES % 4 == 0 && 2 * GZ_WORK_BYTES <= 160 * 1024, "two wavefronts a CU");
ARX_DEVI void gz_carve(GzWork &w, uint8_t *mem) // mem: 16-aligned, GZ_WORK_BYTES
{
	inf_carve(w.inf, mem, nullptr); // (inf.out is not used: the output goes to the ring and the staging span)
	uint8_t *p = mem + ((INF_WORK_BYTES + 15) & ~15);
	w.gs = (int32_t *)p; p += 4 * GS_N;
	w.surv = p; p += INF_LANES;
	w.ring = (uint16_t *)p; // last: the search for candidates does without it (GZ_FIND_BYTES)
}

// where chunk k's symbols go: proportional to the compressed bits in front of its candidate
ARX_HDI int64_t gz_stage_at(int64_t bit, int expand) { return bit * expand / 8; }

// one lane: may a non-final dynamic block start at `pos`?  The fields that fit in registers
ARX_DEVI bool gz_cheap(const uint8_t *ring, int pos, int clen)
{
	InfBits b;
	b.begin(ring, pos);
	if (b.get(3) != 4u) return false; // BFINAL 0, BTYPE 2
	if (b.get(5) > 29u || b.get(5) > 29u) return false;
	const int hclen = (int)b.get(4) + 4;
	if (pos + 17 + 3 * hclen > 8 * clen) return false;
	int kraft = 0;
	for (int i = 0; i < hclen; ++i) { b.refill(); const int l = (int)b.get(3); if (l) kraft += 128 >> l; }
	return kraft == 128;
}

// The first bit of [lo, hi) at which a non-final dynamic block passes inf_header and inf_codes; -1: none.  The reference form of the search: 64
// consecutive positions a round through gz_cheap, the survivors of a round one at a time.  gz_chunk_find calls gz_find_runs below, which gives
// the same position by definition (tests/gzfindsim holds the two together on every chunk's range)
template <class Drv> ARX_DEV int gz_find(Drv &drv, GzWork &w, const uint8_t *src, int clen, int lo, int hi)
{
	InfWork &f = w.inf;
	int32_t *sh = f.sh;
	for (int piece = lo; piece < hi; piece += 8 * GZ_PIECE) {
		bool filled = false;
		const int piece_end = piece + 8 * GZ_PIECE < hi ? piece + 8 * GZ_PIECE : hi;
		for (int round = piece; round < piece_end; round += INF_LANES) {
			if (!filled) {
				drv.lanes([&](int lane) { if (lane == 0) { sh[IS_BITPOS] = piece; sh[IS_HI] = 0; } });
				drv.lanes([&](int lane) { inf_fill(f, src, clen, lane); });
				filled = true;
			}
			drv.lanes([&](int lane) { w.surv[lane] = (uint8_t)(round + lane < piece_end && gz_cheap(f.ring, round + lane, clen)); });
			for (int from = 0; from < INF_LANES;) { // every round moves `from` forward
				drv.lanes([&](int lane) {
					if (lane != 0) return;
					int l = from;
					while (l < INF_LANES && !w.surv[l]) ++l;
					w.gs[GS_PICK] = l;
				});
				const int pick = w.gs[GS_PICK];
				if (pick >= INF_LANES) break;
				drv.lanes([&](int lane) { if (lane == 0) { sh[IS_BITPOS] = round + pick; sh[IS_HI] = 0; sh[IS_STATUS] = INF_OK; sh[IS_OUTPOS] = 0; } });
				drv.lanes([&](int lane) { inf_fill(f, src, clen, lane); });
				drv.lanes([&](int lane) {
					if (lane != 0) return;
					inf_header(f, clen, 0);
					if (sh[IS_STATUS] == INF_OK && sh[IS_BTYPE] == 2 && sh[IS_FINAL] == 0) inf_codes(f);
				});
				filled = false; // the ring holds the candidate's header now
				if (sh[IS_STATUS] == INF_OK && sh[IS_BTYPE] == 2 && sh[IS_FINAL] == 0) return round + pick;
				from = pick + 1;
			}
		}
	}
	return -1;
}

// ---- the same search with a prefilter in front.  A lane takes a run of GZ_RUN consecutive bit positions of the piece in the ring: it reads the
// run's words once, one 32-bit word per 32 positions (the run may start at any bit; a position looks 12 bits ahead), and tests every position in
// registers against the header fields that need no table -- BFINAL 0, BTYPE 2, HLIT <= 29, HDIST <= 29: the first 13 bits, which one position in
// nine passes -- and only a position that passes goes on to gz_cheap's Kraft sum.  What a lane hands on is its first survivor, one word per lane;
// the runs ascend with the lanes, so the least of them is the first survivor of the piece, and one hand-off per piece replaces 256 rounds with
// two each.  The survivors then go to inf_header / inf_codes in ascending order as before; after a refuted one only its lane scans again, from
// the next position (the ring then holds the stream from the refuted position on, which covers the rest of the piece).
constexpr int GZ_RUN = 8 * GZ_PIECE / INF_LANES; // 256 positions
constexpr int GZ_NONE = 0x7FFFFFFF;
static_assert(GZ_RUN * INF_LANES == 8 * GZ_PIECE && GZ_RUN % 32 == 0, "the lanes' runs tile a piece");
// one lane: the first position of [lo, hi) that passes the prefilter and gz_cheap; hi - lo <= GZ_RUN.  GZ_NONE: none
ARX_DEVI int gz_scan(const uint8_t *ring, int lo, int hi, int clen)
{
	if (lo >= hi) return GZ_NONE;
	const uint32_t *r = (const uint32_t *)ring;
	int wpos = lo >> 5;
	uint64_t buf = (uint64_t)r[wpos & (INF_RING / 4 - 1)] | (uint64_t)r[(wpos + 1) & (INF_RING / 4 - 1)] << 32;
	int found = GZ_NONE;
	for (int p0 = 32 * wpos; p0 < hi && found == GZ_NONE; p0 += 32) { // a word of positions at a time, 12 bits of the next word behind them
		for (int b = 0; b < 32; ++b) {
			const int p = p0 + b;
			const uint32_t v = (uint32_t)(buf >> b);
			if (p < lo || p >= hi || found != GZ_NONE || (v & 7u) != 4u || ((v >> 3) & 31u) > 29u || ((v >> 8) & 31u) > 29u) continue;
			if (gz_cheap(ring, p, clen)) found = p;
		}
		++wpos;
		buf = buf >> 32 | (uint64_t)r[(wpos + 1) & (INF_RING / 4 - 1)] << 32;
	}
	return found;
}
template <class Drv> ARX_DEV int gz_find_runs(Drv &drv, GzWork &w, const uint8_t *src, int clen, int lo, int hi)
{
	InfWork &f = w.inf;
	int32_t *sh = f.sh;
	int32_t *first = (int32_t *)f.crc_part; // INF_LANES words the search has no other use for: each lane's first survivor
	for (int piece = lo; piece < hi; piece += 8 * GZ_PIECE) {
		const int piece_end = piece + 8 * GZ_PIECE < hi ? piece + 8 * GZ_PIECE : hi;
		drv.lanes([&](int lane) { if (lane == 0) { sh[IS_BITPOS] = piece; sh[IS_HI] = 0; } });
		drv.lanes([&](int lane) { inf_fill(f, src, clen, lane); });
		drv.lanes([&](int lane) {
			const int a = piece + GZ_RUN * lane, b = a + GZ_RUN < piece_end ? a + GZ_RUN : piece_end;
			first[lane] = gz_scan(f.ring, a, b, clen);
		});
		for (int tries = 0; tries <= 8 * GZ_PIECE; ++tries) { // every refuted survivor moves its lane's entry forward
			drv.lanes([&](int lane) {
				if (lane != 0) return;
				int least = GZ_NONE;
				for (int l = 0; l < INF_LANES; ++l) if (first[l] < least) least = first[l];
				w.gs[GS_PICK] = least;
			});
			const int pick = w.gs[GS_PICK];
			if (pick == GZ_NONE) break;
			drv.lanes([&](int lane) { if (lane == 0) { sh[IS_BITPOS] = pick; sh[IS_HI] = 0; sh[IS_STATUS] = INF_OK; sh[IS_OUTPOS] = 0; } });
			drv.lanes([&](int lane) { inf_fill(f, src, clen, lane); });
			drv.lanes([&](int lane) {
				if (lane != 0) return;
				inf_header(f, clen, 0);
				if (sh[IS_STATUS] == INF_OK && sh[IS_BTYPE] == 2 && sh[IS_FINAL] == 0) inf_codes(f);
			});
			if (sh[IS_STATUS] == INF_OK && sh[IS_BTYPE] == 2 && sh[IS_FINAL] == 0) return pick;
			drv.lanes([&](int lane) { // the ring holds the stream from the refuted position on: the rest of its lane's run lies in it
				if (first[lane] != pick) return;
				const int a = piece + GZ_RUN * lane, b = a + GZ_RUN < piece_end ? a + GZ_RUN : piece_end;
				first[lane] = gz_scan(f.ring, pick + 1, b, clen);
			});
		}
	}
	return -1;
}

// the symbol at output position q of the chunk; q < 0: in front of it
ARX_DEVI uint16_t gz_symbol_at(const uint16_t *ring, int q) { return q < 0 ? (uint16_t)(256 + GZ_WIN + q) : ring[q % GZ_RING]; }
ARX_DEVI void gz_put(GzWork &w, uint16_t *stage, int q, uint16_t s) { w.ring[q % GZ_RING] = s; stage[q] = s; }

ARX_DEV void gz_literals(GzWork &w, uint16_t *stage, int lane)
{
	const InfWork &f = w.inf;
	const int n = f.sh[IS_NLIT], base = f.sh[IS_BASE];
	for (int i = lane; i < n && i < INF_TOK; i += INF_LANES) gz_put(w, stage, base + f.lit_off[i], f.lit_val[i]);
}
ARX_DEV void gz_match(GzWork &w, uint16_t *stage, int k, int lane) // k < IS_NM <= INF_TOK; o + len <= the capacity (inf_decode_t)
{
	const InfWork &f = w.inf;
	const int o = f.sh[IS_BASE] + f.m_off[k], len = f.m_len[k], dist = f.m_dist[k] + 1;
	for (int i = lane; i < len; i += INF_LANES) gz_put(w, stage, o + i, gz_symbol_at(w.ring, o - dist + (dist >= len ? i : i % dist)));
}
// a piece of at most GZ_SPAN bytes of a stored block, from byte `done` of it
ARX_DEV void gz_stored(GzWork &w, const uint8_t *src, uint16_t *stage, int done, int lane)
{
	const int s = w.inf.sh[IS_ST_SRC] + done, d = w.inf.sh[IS_ST_DST] + done, left = w.inf.sh[IS_ST_LEN] - done, n = left < GZ_SPAN ? left : GZ_SPAN;
	for (int i = lane; i < n; i += INF_LANES) gz_put(w, stage, d + i, src[s + i]); // s + n <= clen and d + n <= the capacity (inf_header)
}

// the chunk's blocks from c.cand.  stop: the next chunk's candidate, or -1 where there is none.  stage[0, cap): the chunk's span
template <class Drv> ARX_DEV void gz_decode(Drv &drv, GzWork &w, const uint8_t *src, int clen, int stop, uint16_t *stage, int cap, GzChunk &c)
{
	InfWork &f = w.inf;
	int32_t *sh = f.sh;
	drv.lanes([&](int lane) {
		if (lane != 0) return;
		for (int i = 0; i < IS_N_SCALARS; ++i) sh[i] = 0;
		sh[IS_BITPOS] = c.cand;
	});
	int end_bit = c.cand, count = 0, blocks = 0, flags = 0;
	// a DEFLATE block takes at least 3 bits, a batch at least one: both loops end by the stream's length even before the checks inside do
	for (int round = 0; round <= 8 * clen; ++round) {
		drv.lanes([&](int lane) { inf_fill(f, src, clen, lane); });
		drv.lanes([&](int lane) { if (lane == 0) inf_header(f, clen, cap); });
		if (sh[IS_STATUS] != INF_OK) break;
		if (sh[IS_BTYPE] == 0) {
			for (int done = 0; done < sh[IS_ST_LEN]; done += GZ_SPAN) drv.lanes([&](int lane) { gz_stored(w, src, stage, done, lane); });
		} else {
			if (sh[IS_BTYPE] == 1) drv.lanes([&](int lane) { inf_fixed_lengths(f, lane); });
			drv.lanes([&](int lane) {
				if (lane == 0) inf_codes(f);
				inf_table_clear(f.ll_tab, INF_LL_BITS, lane); inf_table_clear(f.d_tab, INF_D_BITS, lane);
			});
			if (sh[IS_STATUS] != INF_OK) break;
			drv.lanes([&](int lane) {
				inf_table_fill(f.ll_tab, INF_LL_BITS, f.len, f.first, f.index, f.sym, sh[IS_NSYM_LL], lane);
				inf_table_fill(f.d_tab, INF_D_BITS, f.len + INF_LL, f.first + 16, f.index + 16, f.sym + INF_LL, sh[IS_NSYM_D], lane);
			});
			for (int batches = 0; batches <= 8 * clen; ++batches) {
				drv.lanes([&](int lane) { inf_fill(f, src, clen, lane); });
				drv.lanes([&](int lane) { if (lane == 0) inf_decode_t<true>(f, clen, cap, GZ_SPAN); });
				if (sh[IS_STATUS] != INF_OK) break;
				drv.lanes([&](int lane) { gz_literals(w, stage, lane); });
				const int nm = sh[IS_NM] < INF_TOK ? sh[IS_NM] : INF_TOK;
				for (int k = 0; k < nm; ++k) drv.lanes([&](int lane) { gz_match(w, stage, k, lane); });
				if (sh[IS_EOB]) break;
			}
			if (sh[IS_STATUS] != INF_OK || !sh[IS_EOB]) break;
		}
		end_bit = sh[IS_BITPOS]; count = sh[IS_OUTPOS]; ++blocks; // a completed block: what a later, cut off one produces is dropped
		if (sh[IS_FINAL]) { flags |= GZ_F_MEMBER_END; break; }
		if (stop >= 0 && end_bit >= stop) { flags |= end_bit == stop ? GZ_F_CONFIRMED : GZ_F_PASSED; break; }
	}
	const int st = sh[IS_STATUS];
	c.end_bit = end_bit; c.count = count; c.blocks = blocks; c.flags = flags; c.inf = st;
	// the bytes ran out inside a block: what was completed stands.  The capacity ran out: inf_header and inf_decode_t call that a size mismatch
	c.status = st == INF_OK || (st == INF_TRUNCATED && blocks > 0) ? GZ_OK : st == INF_TRUNCATED ? GZ_NO_BLOCK : st == INF_SIZE_MISMATCH ? GZ_OVERFLOW : GZ_BAD_STREAM;
}

// one wavefront's share of the first two phases: chunk k of n.  Two launches on the GPU (every candidate is needed before a decode knows where
// to stop), so `decode` says which half this is
template <class Drv> ARX_DEV void gz_chunk_find(Drv &drv, GzWork &w, const uint8_t *src, int clen, int chunk_bytes, int start_bit, int k, GzChunk &c)
{
	const int64_t lo = 8 * (int64_t)k * chunk_bytes, hi = lo + 8 * (int64_t)chunk_bytes < 8 * (int64_t)clen ? lo + 8 * (int64_t)chunk_bytes : 8 * (int64_t)clen;
	c.cand = k == 0 ? start_bit : gz_find_runs(drv, w, src, clen, (int)lo, (int)hi);
	c.next = 0; c.end_bit = c.cand; c.count = 0; c.status = GZ_NO_CANDIDATE; c.inf = 0; c.flags = 0; c.blocks = 0; c.order = -1; c.bad_markers = 0; c.crc = 0; c.markers = 0; c.have = 0; c.pad = 0;
	c.stage_off = c.stage_cap = c.text_off = 0;
}
template <class Drv> ARX_DEV void gz_chunk_decode(Drv &drv, GzWork &w, const uint8_t *src, int clen, int expand, int k, int n, GzChunk *chunks, uint16_t *stage)
{
	GzChunk c = chunks[k];
	if (c.cand < 0) return;
	int next = k + 1;
	while (next < n && chunks[next].cand < 0) ++next;
	c.next = next;
	const int stop = next < n ? chunks[next].cand : -1;
	c.stage_off = gz_stage_at(c.cand, expand);
	c.stage_cap = gz_stage_at(next < n ? stop : 8 * (int64_t)clen, expand) - c.stage_off;
	if (c.stage_cap < 0) c.stage_cap = 0;
	if (c.stage_cap > GZ_MAX_SYMBOLS) c.stage_cap = GZ_MAX_SYMBOLS;
	gz_decode(drv, w, src, clen, stop, stage + c.stage_off, (int)c.stage_cap, c);
	drv.lanes([&](int lane) { // its results only: `cand` is read by the other chunks of this launch, and stays the search's
		if (lane != 0) return;
		GzChunk &o = chunks[k];
		o.next = c.next; o.end_bit = c.end_bit; o.count = c.count; o.status = c.status; o.inf = c.inf; o.flags = c.flags; o.blocks = c.blocks;
		o.stage_off = c.stage_off; o.stage_cap = c.stage_cap;
	});
}

// one lane: the accepted chain, every accepted chunk's place in it and in the text.  have: bytes of the carried window that exist
ARX_DEV void gz_chain(GzChunk *chunks, int n, int have, GzChain &out)
{
	int64_t text = 0;
	int m = 0, last = -1;
	for (int k = 0; k >= 0 && k < n && m < n;) { // k only grows
		GzChunk &c = chunks[k];
		if (c.cand < 0 || c.status != GZ_OK) break;
		c.flags |= GZ_F_ACCEPTED; c.order = m; c.text_off = text; c.have = have;
		text += c.count; ++m; last = k;
		have = c.count >= GZ_WIN - have ? GZ_WIN : have + c.count;
		if ((c.flags & GZ_F_MEMBER_END) || !(c.flags & GZ_F_CONFIRMED) || c.next <= k) break;
		k = c.next;
	}
	out.n_accepted = m; out.last = last; out.have = have; out.pad = 0; out.text_bytes = text;
}

// entry i of the window behind a chunk of `count` symbols: the last 32 KiB of (prev followed by the chunk's bytes)
ARX_DEVI void gz_window_at(const uint8_t *prev, uint8_t *next, const uint16_t *sym, int count, int i)
{
	const int64_t t = (int64_t)count + i; // its place in the two laid end to end
	if (t < GZ_WIN) { next[i] = prev[t]; return; }
	const uint16_t s = sym[t - GZ_WIN];
	next[i] = s < 256 ? (uint8_t)s : prev[(s - 256) & (GZ_WIN - 1)];
}
// is symbol i of a chunk a marker that names a byte in front of the `have` the window holds?  (have < GZ_WIN: the first 32 KiB of a member)
ARX_DEVI bool gz_bad_marker_at(const uint16_t *sym, int have, int64_t i)
{
	const uint16_t s = sym[i];
	return s >= 256 && ((s - 256) & (GZ_WIN - 1)) < GZ_WIN - have;
}
// byte i of a chunk to its place; -> was it a marker
ARX_DEVI bool gz_resolve_at(const uint8_t *win, const uint16_t *sym, uint8_t *text, int64_t i)
{
	const uint16_t s = sym[i];
	text[i] = s < 256 ? (uint8_t)s : win[(s - 256) & (GZ_WIN - 1)];
	return s >= 256;
}
// the CRC tables of inf_begin, by any number of lanes
ARX_DEV void gz_crc_tables(uint32_t *crc_tab, uint32_t *x2n, int lane, int lanes)
{
	for (int i = lane; i < 256; i += lanes) {
		uint32_t c = (uint32_t)i;
		for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ BGZF_POLY : c >> 1;
		crc_tab[i] = c;
	}
	if (lane == 0) {
		uint32_t p = 0x40000000u; // x^1
		x2n[0] = p;
		for (int k = 1; k < 32; ++k) { p = bgzf_gf_mul(p, p); x2n[k] = p; }
	}
}
// part t of T of the CRC-32 of text[0, n)
ARX_DEVI uint32_t gz_crc_part(const uint32_t *crc_tab, const uint32_t *x2n, const uint8_t *text, int64_t n, int t, int T)
{
	const int64_t per = (n + T - 1) / T, s = t * per < n ? t * per : n, e = s + per < n ? s + per : n;
	return inf_crc_range(crc_tab, x2n, [&](int64_t p) { return text[p]; }, s, e, n);
}

} // namespace arx

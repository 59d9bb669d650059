// dev_bamsort.h -- the coordinate sort of one BAM record stream as launches over an explicit item index: where the records start, their keys,
// and the gather of the sorted records.  hip_bamsort.h runs the functors below as kernels, one item per thread, and the key sort through
// rocprim; tests/sortsim/bam_sort_sim.cpp runs the very same functions on the host, the items of a launch in a loop, in either order, with
// std::stable_sort for the key sort.  Nothing here knows which of the two it is: a driver `drv` supplies
//     drv.items(name, n, f)                         f(i) for every i in [0, n), in any order, all done when the next call starts
//     drv.scan(in, out, n)                          out[0..n]: the exclusive prefix sums of in[0..n), out[n] the total
//     drv.get(p) / drv.put(p, v)                    one int64 of the launches' memory, read or written by the host
//     drv.sort_pairs(kin, kout, vin, vout, n, bits) a STABLE sort of n (key, value) pairs by the low `bits` bits of the key
//
// Record discovery.  A BAM record stream is a chain: a record at o, the next at o + 4 + block_size.  Following it is serial, so the stream
// behind the header is cut into segments of seg bytes (a power of two, at least BS_MIN_SEG) that are walked side by side:
//   probe    every segment but the first looks for the first offset inside it at which a record could start: the fixed fields are in range
//            (bs_check), the variable parts fit into block_size, the record lies inside the stream, and the same holds for the
//            BS_PROBE_DEPTH - 1 records the chain leads to.  That is guess[s], or none
//   walk     every segment follows the chain from its entry (segment 0: the header's end; the others: their guess) until the offset
//            reaches the segment's end: cnt[s] record starts, and exit[s], the first chain offset at or behind the next segment's start
//            (it may lie several segments on: a record may be longer than a segment)
//   verify   segment s is right exactly when its entry equals exit[s - 1] and segment s - 1 is right; segment 0 is right by construction.
//            A round re-walks every segment whose entry differs from its predecessor's exit of the round before (the two states are
//            double-buffered, so a round reads nothing it writes); rounds repeat until none differs.  Every round makes at least the
//            first wrong segment right, so there are at most n_seg rounds; where every guess was right there is one, and it walks nothing.
//            A segment whose entry lies at or behind its end holds no record start: no records, and the exit passes the entry on
//   fill     the counts' prefix sums say where a segment's record offsets go; every segment walks once more and writes them
// What the probe guesses therefore only decides how much is re-walked, never the result: a fake chain inside a record's payload gives an
// entry that differs from the predecessor's exit -- also where the fake chain rejoins the true one -- and is walked again from the true one.
//
// Bounds.  Every step of a walk checks o + 4 <= n, block_size >= 32 and o + 4 + block_size <= n before it reads on, and a walk ends by a step
// count derived from the segment's size (block_size >= 32: a step moves on by at least 36 bytes), not by the data.  A walk from a wrong entry
// that breaks stops there, in bounds, with the exit BS_BROKEN; its successor takes that over until the round that replaces both.  BS_BROKEN
// that survives verification is on the true chain: the input's error.
//
// A slab (copy mode: arx_bam_sort_append hands a file on in slabs of whole BGZF blocks, which end anywhere in a record): `open` set, the
// stream's end is not the chain's.  A block_size field cut by the end stops the walk in front of it -- the exit is that offset, and the next
// slab carries the BS_SLAB_KEEP bytes in front of its own so that the field is whole there; a record that runs past the end counts, its exit
// lies behind the end.  The exit of the last segment is what the next slab's segment 0 enters at (bs_slab_entry).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "arx_hd.h"

namespace arx {

constexpr int64_t BS_MIN_SEG = 64;
constexpr int BS_PROBE_DEPTH = 4;       // records a guess must chain through (fewer where the stream ends first)
constexpr int BS_GATHER_LANES = 16;     // lanes that copy one record
constexpr int BS_SLAB_KEEP = 3;         // bytes of the slab before in front of a slab: a cut block_size field is at most that long
constexpr int64_t BS_NONE = -1, BS_BROKEN = -2;
enum { BS_OK = 0, BS_E_CHAIN = 1 };
enum { BS_C_DIFFER = 0, BS_C_RIGHT, BS_N_COUNTERS };

struct BsStream {
	const uint8_t *s; int64_t n; // the bytes
	int64_t hdr;                 // where the first record starts (segment 0's entry); hdr >= n: no segment
	int64_t seg;
	int32_t n_ref, open;
};
ARX_HDI int64_t bs_n_seg(const BsStream &t) { return t.hdr < t.n ? (t.n - t.hdr + t.seg - 1) / t.seg : 0; }
ARX_HDI int64_t bs_seg_lo(const BsStream &t, int64_t s) { return t.hdr + s * t.seg; }
ARX_HDI int64_t bs_seg_hi(const BsStream &t, int64_t s) { const int64_t hi = t.hdr + (s + 1) * t.seg; return hi < t.n ? hi : t.n; }

// a record may start at any byte: its words are read byte by byte
ARX_HDI uint32_t bs_r32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// Could a record start at o?  -> the offset behind it; BS_NONE: no; BS_BROKEN (open streams only): the stream ends before that can be said
ARX_DEVI int64_t bs_check(const BsStream &t, int64_t o)
{
	if (o + 36 > t.n) return t.open ? BS_BROKEN : BS_NONE;
	const uint8_t *p = t.s + o;
	const int64_t bs = (int64_t)bs_r32(p);
	if (bs < 32 || bs > INT32_MAX) return BS_NONE;
	const int32_t rid = (int32_t)bs_r32(p + 4), pos = (int32_t)bs_r32(p + 8), l_seq = (int32_t)bs_r32(p + 20), mrid = (int32_t)bs_r32(p + 24), mpos = (int32_t)bs_r32(p + 28);
	const int64_t l_name = p[12], n_cig = (int64_t)p[16] | (int64_t)p[17] << 8;
	if (rid < -1 || rid >= t.n_ref || mrid < -1 || mrid >= t.n_ref || pos < -1 || mpos < -1 || l_seq < 0 || l_name < 2) return BS_NONE;
	if (32 + l_name + 4 * n_cig + ((int64_t)l_seq + 1) / 2 + l_seq > bs) return BS_NONE;
	if (o + 36 + l_name > t.n) return t.open ? BS_BROKEN : BS_NONE;
	if (p[36 + l_name - 1] != 0) return BS_NONE;
	if (o + 4 + bs > t.n && !t.open) return BS_NONE;
	return o + 4 + bs;
}
// the guess of a segment: the first offset in [lo, hi) from which BS_PROBE_DEPTH records chain, or fewer where the stream ends with one
ARX_DEVI int64_t bs_probe(const BsStream &t, int64_t lo, int64_t hi)
{
	for (int64_t o = lo; o < hi; ++o) {
		int64_t at = o;
		bool ok = true;
		for (int d = 0; d < BS_PROBE_DEPTH; ++d) {
			if (at >= t.n) { ok = d > 0 && (t.open || at == t.n); break; } // the chain left the stream: at its end, or anywhere where the end is open
			const int64_t nx = bs_check(t, at);
			if (nx == BS_BROKEN) { ok = d > 0; break; }
			if (nx < 0) { ok = false; break; }
			at = nx;
		}
		if (ok) return o;
	}
	return BS_NONE;
}

struct BsWalked { int64_t cnt, exit; };
// the chain from o until it reaches hi (a segment's end, hi <= n); out (may be null): where the record starts go
ARX_DEVI BsWalked bs_walk(const BsStream &t, int64_t o, int64_t hi, int64_t *out)
{
	BsWalked r = {0, o};
	if (o >= hi) return r; // no record start in here: the entry is passed on
	const int64_t steps = (hi - o) / 36 + 1;
	for (int64_t k = 0; k < steps && o < hi; ++k) {
		if (o + 4 > t.n) {
			if (t.open) break; // the field is cut: the next slab reads it
			r.exit = BS_BROKEN; return r;
		}
		const int64_t bs = (int64_t)bs_r32(t.s + o);
		if (bs < 32 || (!t.open && o + 4 + bs > t.n)) { r.exit = BS_BROKEN; return r; }
		if (out) out[r.cnt] = o;
		++r.cnt;
		o += 4 + bs;
	}
	r.exit = o;
	return r;
}

// ---- the launches of the discovery, one segment per item
struct BsSegState { int64_t *entry, *exit, *cnt; };

struct BsProbeF {
	BsStream t; int64_t *guess;
	ARX_DEVI void operator()(int64_t s) const { guess[s] = s == 0 ? t.hdr : bs_probe(t, bs_seg_lo(t, s), bs_seg_hi(t, s)); }
};
struct BsWalkF { // the first walk: from the guess
	BsStream t; const int64_t *guess; BsSegState st;
	ARX_DEVI void operator()(int64_t s) const
	{
		const int64_t e = guess[s];
		BsWalked w = {0, BS_NONE};
		if (e >= 0) w = bs_walk(t, e, bs_seg_hi(t, s), nullptr);
		st.entry[s] = e; st.exit[s] = w.exit; st.cnt[s] = w.cnt;
	}
};
struct BsVerifyF { // one round: `in` is the state of the round before, `out` this round's
	BsStream t; BsSegState in, out; int64_t *counters;
	ARX_DEVI void operator()(int64_t s) const
	{
		const int64_t want = s == 0 ? t.hdr : in.exit[s - 1], e = in.entry[s];
		if (want == e && e != BS_NONE) { out.entry[s] = e; out.exit[s] = in.exit[s]; out.cnt[s] = in.cnt[s]; return; }
		ARX_ATOMIC_ADD64(&counters[BS_C_DIFFER], 1);
		if (want == BS_NONE) { out.entry[s] = e; out.exit[s] = in.exit[s]; out.cnt[s] = in.cnt[s]; return; } // the predecessor does not know yet
		BsWalked w = {0, BS_BROKEN};
		if (want >= 0) w = bs_walk(t, want, bs_seg_hi(t, s), nullptr);
		out.entry[s] = want; out.exit[s] = w.exit; out.cnt[s] = w.cnt;
	}
};
struct BsTallyF { // the guesses that were right: the verified entry, or none where the segment holds no record start
	BsStream t; const int64_t *guess; BsSegState st; int64_t *counters;
	ARX_DEVI void operator()(int64_t i) const
	{
		const int64_t s = i + 1, g = guess[s], e = st.entry[s];
		if (g == e || (g == BS_NONE && e >= bs_seg_hi(t, s))) ARX_ATOMIC_ADD64(&counters[BS_C_RIGHT], 1);
	}
};
struct BsFillF {
	BsStream t; BsSegState st; const int64_t *base; int64_t *rec_off;
	ARX_DEVI void operator()(int64_t s) const { if (st.entry[s] >= 0) bs_walk(t, st.entry[s], bs_seg_hi(t, s), rec_off + base[s]); }
};

// the work memory of a discovery over at most n_seg segments, in int64 words: guess, two states of three arrays, the scan's n_seg + 1, the counters
ARX_HDI int64_t bs_seg_words(int64_t n_seg) { return 8 * n_seg + 1 + BS_N_COUNTERS; }
struct BsSegs {
	int64_t *guess, *base, *counters;
	BsSegState st[2];
	int cur = 0; // the state that holds
	void carve(int64_t *mem, int64_t n_seg)
	{
		guess = mem; mem += n_seg;
		for (int k = 0; k < 2; ++k) { st[k].entry = mem; mem += n_seg; st[k].exit = mem; mem += n_seg; st[k].cnt = mem; mem += n_seg; }
		base = mem; mem += n_seg + 1;
		counters = mem;
	}
};
struct BsFound { int64_t n_records, exit, n_seg, right, repaired, rounds; };

// probe, walk, verify and repair -> BS_OK and what was found (the record count; exit: where the chain leaves the stream, n unless `open`), or
// BS_E_CHAIN: the chain breaks, or does not end with the stream.  Nothing is written but w's memory
template <class Drv> int bs_discover(Drv &drv, const BsStream &t, BsSegs &w, BsFound *f)
{
	const int64_t ns = bs_n_seg(t);
	*f = BsFound{0, t.hdr, ns, 0, 0, 0};
	if (ns == 0) return t.open || t.hdr == t.n ? BS_OK : BS_E_CHAIN;
	drv.items("bs_probe", ns, BsProbeF{t, w.guess});
	w.cur = 0;
	drv.items("bs_walk", ns, BsWalkF{t, w.guess, w.st[0]});
	for (int64_t round = 0;; ++round) {
		if (round > ns) return BS_E_CHAIN; // cannot happen: a round makes the first wrong segment right
		drv.put(&w.counters[BS_C_DIFFER], 0);
		drv.items("bs_verify", ns, BsVerifyF{t, w.st[w.cur], w.st[w.cur ^ 1], w.counters});
		w.cur ^= 1;
		if (drv.get(&w.counters[BS_C_DIFFER]) == 0) break;
		++f->rounds;
	}
	const BsSegState &st = w.st[w.cur];
	f->exit = drv.get(&st.exit[ns - 1]);
	if (f->exit == BS_BROKEN || (!t.open && f->exit != t.n)) return BS_E_CHAIN;
	drv.scan(st.cnt, w.base, ns);
	f->n_records = drv.get(&w.base[ns]);
	drv.put(&w.counters[BS_C_RIGHT], 0);
	if (ns > 1) drv.items("bs_tally", ns - 1, BsTallyF{t, w.guess, st, w.counters});
	f->right = drv.get(&w.counters[BS_C_RIGHT]);
	f->repaired = ns - 1 - f->right;
	return BS_OK;
}
// after bs_discover returned BS_OK: rec_off[0 .. n_records] (the last entry is the exit)
template <class Drv> void bs_fill(Drv &drv, const BsStream &t, BsSegs &w, const BsFound &f, int64_t *rec_off)
{
	if (f.n_seg) drv.items("bs_fill", f.n_seg, BsFillF{t, w.st[w.cur], w.base, rec_off});
	drv.put(&rec_off[f.n_records], f.exit);
}

// slabs: slab [a, b) of a stream is handed over as the bytes [a - bs_slab_keep(a), b); where the chain enters it, given the exit so far
ARX_HDI int64_t bs_slab_keep(int64_t a) { return a < BS_SLAB_KEEP ? a : BS_SLAB_KEEP; }
ARX_HDI int64_t bs_slab_entry(int64_t a, int64_t exit_so_far) { return exit_so_far - (a - bs_slab_keep(a)); }
struct BsCarry { int64_t exit, n_records, n_seg, right, repaired, rounds; }; // exit: starts as the header's end; the sums over the slabs so far
// one slab: buf holds the stream's bytes [a - bs_slab_keep(a), b).  BS_OK: c is moved on; after the last slab c.exit must be the stream's size
template <class Drv> int bs_count_slab(Drv &drv, const uint8_t *buf, int64_t a, int64_t b, int64_t seg, int32_t n_ref, BsSegs &w, BsCarry &c)
{
	const int64_t keep = bs_slab_keep(a);
	const BsStream t = {buf, b - a + keep, bs_slab_entry(a, c.exit), seg, n_ref, 1};
	BsFound f;
	if (t.hdr < 0 || bs_discover(drv, t, w, &f) != BS_OK) return BS_E_CHAIN;
	c.exit = a - keep + f.exit; c.n_records += f.n_records; c.n_seg += f.n_seg; c.right += f.right; c.repaired += f.repaired; c.rounds += f.rounds;
	return BS_OK;
}

// ---- keys: one record per item.  ((uint32_t)refID, pos) in 64 bits: refID = -1 (and whatever else lies outside [0, n_ref)) becomes n_ref, so
// that it sorts last and the key needs 32 + bits(n_ref) bits; pos + 1 keeps the signed order of pos >= -1 in an unsigned word
ARX_HDI int bs_key_bits(int32_t n_ref) { int b = 0; while (b < 31 && ((int64_t)1 << b) <= (int64_t)n_ref) ++b; return 32 + b; }
struct BsKeysF {
	const uint8_t *s; const int64_t *rec_off; int32_t n_ref; uint64_t *keys; uint32_t *vals;
	ARX_DEVI void operator()(int64_t j) const
	{
		const uint8_t *p = s + rec_off[j];
		const int32_t rid = (int32_t)bs_r32(p + 4), pos = (int32_t)bs_r32(p + 8);
		const uint32_t r = rid < 0 || rid >= n_ref ? (uint32_t)n_ref : (uint32_t)rid;
		keys[j] = (uint64_t)r << 32 | (uint32_t)(pos + 1u);
		vals[j] = (uint32_t)j;
	}
};

// ---- gather: the sizes of the records in sorted order, their prefix sums, then BS_GATHER_LANES lanes copy each record to its place
struct BsSizesF {
	const int64_t *rec_off; const uint32_t *vals; int64_t *size;
	ARX_DEVI void operator()(int64_t j) const { const int64_t v = vals[j]; size[j] = rec_off[v + 1] - rec_off[v]; }
};
// lane `lane` of `lanes`: its share of dst[0, len) = src[0, len).  The two alignments are independent: whole words are stored at the
// destination's alignment and loaded from wherever that puts them in the source
ARX_DEVI void bs_copy(uint8_t *dst, const uint8_t *src, int64_t len, int lane, int lanes)
{
	int64_t head = (int64_t)((8 - ((uintptr_t)dst & 7)) & 7);
	if (head > len) head = len;
	for (int64_t k = lane; k < head; k += lanes) dst[k] = src[k];
	const int64_t nw = (len - head) / 8;
	for (int64_t k = lane; k < nw; k += lanes) {
		uint64_t x;
		memcpy(&x, src + head + 8 * k, 8);
		memcpy(__builtin_assume_aligned(dst + head + 8 * k, 8), &x, 8);
	}
	for (int64_t k = head + 8 * nw + lane; k < len; k += lanes) dst[k] = src[k];
}
struct BsGatherF {
	const uint8_t *src; uint8_t *dst; const int64_t *rec_off; const uint32_t *vals; const int64_t *out_off;
	ARX_DEVI void operator()(int64_t i) const
	{
		const int64_t j = i / BS_GATHER_LANES, v = vals[j];
		bs_copy(dst + out_off[j], src + rec_off[v], rec_off[v + 1] - rec_off[v], (int)(i % BS_GATHER_LANES), BS_GATHER_LANES);
	}
};

// the work memory of the sort of n records behind the discovery, in bytes: rec_off and out_off (n + 1 each), sizes, two key and two value arrays
ARX_HDI int64_t bs_sort_bytes(int64_t n) { return 8 * (3 * n + 2) + 16 * n + 8 * n + 64; }
struct BsSortMem { int64_t *size, *out_off; uint64_t *keys[2]; uint32_t *vals[2]; };

// keys, sort, sizes, scan, gather: dst[0, n) = the records of s in key order, equal keys in stream order; m.out_off[0 .. n_records]: where they start
template <class Drv> void bs_sort_gather(Drv &drv, const uint8_t *s, const int64_t *rec_off, int64_t n_records, int32_t n_ref, BsSortMem &m, uint8_t *dst)
{
	if (n_records == 0) { drv.put(&m.out_off[0], 0); return; }
	drv.items("bs_keys", n_records, BsKeysF{s, rec_off, n_ref, m.keys[0], m.vals[0]});
	drv.sort_pairs(m.keys[0], m.keys[1], m.vals[0], m.vals[1], n_records, bs_key_bits(n_ref));
	drv.items("bs_sizes", n_records, BsSizesF{rec_off, m.vals[1], m.size});
	drv.scan(m.size, m.out_off, n_records);
	drv.items("bs_gather", n_records * BS_GATHER_LANES, BsGatherF{s, dst, rec_off, m.vals[1], m.out_off});
}

// ---- the BAM header in front of the records, parsed by the host from the first inflated bytes.  1: *end is where the records start and the
// references were handed to ref(i, name, l_name_with_nul, l_ref); 0: more than the n bytes given are needed (*end: how many at least); -1: not a BAM header
template <class Ref> inline int bs_parse_header(const uint8_t *p, int64_t n, int64_t *end, int32_t *n_ref, Ref ref)
{
	*end = 12;
	if (n < 12) return 0;
	if (p[0] != 'B' || p[1] != 'A' || p[2] != 'M' || p[3] != 1) return -1;
	const int64_t l_text = (int32_t)bs_r32(p + 4);
	if (l_text < 0) return -1;
	int64_t o = 8 + l_text;
	*end = o + 4;
	if (n < o + 4) return 0;
	const int32_t nr = (int32_t)bs_r32(p + o);
	if (nr < 0) return -1;
	o += 4;
	for (int32_t i = 0; i < nr; ++i) {
		*end = o + 4;
		if (n < o + 4) return 0;
		const int64_t l = (int32_t)bs_r32(p + o);
		if (l < 1) return -1;
		*end = o + 4 + l + 4;
		if (n < o + 4 + l + 4) return 0;
		ref(i, (const char *)p + o + 4, l, (int32_t)bs_r32(p + o + 4 + l));
		o += 4 + l + 4;
	}
	*end = o;
	*n_ref = nr;
	return 1;
}

} // namespace arx

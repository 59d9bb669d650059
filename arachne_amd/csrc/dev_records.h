// dev_records.h -- the primary BAM record of every read, encoded on the device: what RecBuf::build's first mode (bam_records.h) followed by
// BamSink::encode (bam_sink.h) writes, as functors over the arrays a placed batch has in HBM.  Every rule of the record's fields -- active
// candidate, unmapped, flags, mapq, TempLen, CIGAR ops, bin, aux length, the fixed part -- is bam_rules.h's, shared with those two; what is
// stated here is where each byte of the stream comes from (rec_byte):
//   name, CIGAR        the name NUL-terminated; bam_cigar_word of the alignment's words, none for the placeholder (reg < 0)
//   bases              4-bit codes of ACGTN (1, 2, 4, 8, 15), high nibble first, complemented and reversed for a reverse-strand candidate; an odd
//                      length leaves a zero low nibble.  Qualities minus 33, reversed likewise (bamwriter.go:372-375)
//   aux                RG:Z (only a non-empty read group), AS:i as int32, XM:Z:0, AM:Z:0|1, XT:C:0, BX:Z + VX:C:1 for a set with bam_set_bx
// A read without an active candidate raises REC_ERR_NO_ACTIVE.  Compiled for the device and for the host test double.
//
// Launch order (pipeline_records.h), every functor through launch_wide:
//   KBamRecSize    one read per lane: the active candidates of the read and its mate, the record's size and where its parts begin, its
//               finished 36-byte fixed part (RecMeta: the fill searches nothing again)                    -> scan -> record offsets
//   KBamRecTile    one 256-byte tile of the stream per lane: the first record that ends beyond the tile's start (one binary search)
//   KBamRecFill    one aligned 16-byte word of the stream per lane, see there
#pragma once
#include "arx_dev.h"
#include "bam_rules.h"
#include "dev_rfa.h"
#include "dev_post.h"

namespace arx {

enum : uint32_t { REC_ERR_NO_ACTIVE = 1 };
constexpr int REC_TILE = 256;       // bytes of the stream per entry of the tile table

struct alignas(16) RecWord16 { uint32_t w[4]; };

// what the caller's arx_super_batch adds to the batch, in device memory (uploaded by the records call)
struct RecInputs {
	const uint8_t *quals;                                 // one byte per base, laid out as the batch's bases
	const uint8_t *names; const int64_t *name_off;        // per pair
	const uint8_t *rgs; const int64_t *rg_off;            // per pair
	const uint8_t *barcodes; const int64_t *barcode_off;  // per set
	const int64_t *set_pair_off; const uint8_t *set_bx;   // per set: its pairs; 1 = its records carry BX / VX
	int32_t n_sets;
};

// per record: sizes and starts of its parts (byte offsets from the record's first byte) and its fixed part (bam_fixed)
struct RecMeta {
	uint32_t fixed[9];
	int32_t size;                 // whole record, block_size included
	int32_t o_cig, o_seq, o_qual, o_aux; // name starts at 36
	int32_t cig_src;              // first CIGAR word of the candidate's alignment in the batch's CIGAR array
	int32_t l_seq, base_off;
	int32_t bits;                 // 1: reverse strand, 2: active molecule, 4: BX / VX
	int32_t score, set, rgl, bcl;
	int32_t pad[2];
};
static_assert(sizeof(RecMeta) == 96, "RecMeta is read as six 16-byte words");

struct KBamRecSize {
	const Cand *cands; const int32_t *cand_off; const Aln *alns; const uint32_t *cig; const CandPost *post; // post: null = no duplicate flags
	const int32_t *lens, *base_off; RecInputs in;
	RecMeta *meta; int32_t *size; uint32_t *err;
	ARX_DEV void operator()(int r, int) const
	{
		int a = bam_active(cands, cand_off, r), am = bam_active(cands, cand_off, r ^ 1);
		if (a < 0) { ARX_ATOMIC_OR(err, REC_ERR_NO_ACTIVE); a = cand_off[r]; }
		if (am < 0) am = cand_off[r ^ 1]; // (the mate's own lane raises the bit)
		const Cand &c = cands[a], &m = cands[am];
		const int p = r >> 1;
		int lo = 0, hi = in.n_sets; // the set of pair p: the last one that starts at or before it
		while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (in.set_pair_off[mid] <= p) lo = mid; else hi = mid; }
		const int s = lo;
		const bool un = bam_unmapped(c), mun = bam_unmapped(m);
		const uint32_t fl = bam_flag(r & 1, c.is_proper, un, mun, m.reversed, c.reversed, post && post[a].duplicate, false);
		const int32_t rid = un ? -1 : c.rid, pos = un ? -1 : (int32_t)c.pos;
		const uint32_t mapq = un ? 0u : bam_mapq(c.mapq);
		const int32_t tl = bam_tlen(c, m, c.pos, m.pos);
		const int n_cig = c.reg >= 0 ? alns[c.reg].n_cigar : 0, cig_src = c.reg >= 0 ? alns[c.reg].cigar_off : 0;
		const int bin = bam_bin(pos, bam_ref_len(cig + cig_src, n_cig, true));
		const int l_name = (int)(in.name_off[p + 1] - in.name_off[p]) + 1, L = lens[r];
		const int rgl = (int)(in.rg_off[p + 1] - in.rg_off[p]), bcl = (int)(in.barcode_off[s + 1] - in.barcode_off[s]);
		const bool bx = in.set_bx[s] != 0;
		RecMeta t;
		t.o_cig = 36 + l_name; t.o_seq = t.o_cig + 4 * n_cig; t.o_qual = t.o_seq + (L + 1) / 2; t.o_aux = t.o_qual + L; t.size = t.o_aux + bam_first_aux_len(rgl, bx, bcl);
		bam_fixed(t.fixed, t.size, rid, pos, (uint32_t)l_name, mapq, bin, (uint32_t)n_cig, fl, (uint32_t)L, mun ? -1 : m.rid, mun ? -1 : (int32_t)m.pos, tl);
		t.cig_src = cig_src; t.l_seq = L; t.base_off = base_off[r];
		t.bits = (c.reversed ? 1 : 0) | (c.active_molecule ? 2 : 0) | (bx ? 4 : 0);
		t.score = c.score; t.set = s; t.rgl = rgl; t.bcl = bcl; t.pad[0] = t.pad[1] = 0;
		meta[r] = t; size[r] = t.size;
	}
};

// tile t covers stream bytes [t * REC_TILE, (t + 1) * REC_TILE): first[t] = the first record that ends beyond t * REC_TILE, the record of the
// tile's first byte.  Every tile starts inside the stream, so the record exists
struct KBamRecTile {
	const int32_t *rec_off; int n_rec; int32_t *first;
	ARX_DEV void operator()(int t, int) const
	{
		const int64_t b = (int64_t)t * REC_TILE;
		int lo = 0, hi = n_rec; // smallest r with rec_off[r + 1] > b
		while (lo < hi) { const int mid = (lo + hi) >> 1; if ((int64_t)rec_off[mid + 1] > b) hi = mid; else lo = mid + 1; }
		first[t] = lo;
	}
};

// byte `off` of record r (meta t): a function of (record, offset) alone
struct RecSources { const uint32_t *cig; const uint8_t *bases; RecInputs in; };
ARX_DEVI uint32_t rec_base4(const RecSources &S, const RecMeta &t, int i) // 4-bit code of base i of the record as written
{
	const bool rev = t.bits & 1;
	const uint32_t y = S.bases[t.base_off + (rev ? t.l_seq - 1 - i : i)];
	if (y > 3) return 15u;
	return 1u << (rev ? 3 - y : y); // A C G T = 1 2 4 8; the complement mirrors them
}
ARX_DEVI uint32_t rec_byte(const RecSources &S, const RecMeta &t, int r, int off)
{
	if (off < 36) return (t.fixed[off >> 2] >> (8 * (off & 3))) & 0xffu;
	const int p = r >> 1;
	if (off < t.o_cig) return off == t.o_cig - 1 ? 0u : S.in.names[S.in.name_off[p] + (off - 36)];
	if (off < t.o_seq) { const int k = off - t.o_cig; return (bam_cigar_word(S.cig[t.cig_src + (k >> 2)]) >> (8 * (k & 3))) & 0xffu; }
	if (off < t.o_qual) { const int i = 2 * (off - t.o_seq); return rec_base4(S, t, i) << 4 | (i + 1 < t.l_seq ? rec_base4(S, t, i + 1) : 0u); }
	if (off < t.o_aux) { const int i = off - t.o_qual; return (uint32_t)(uint8_t)(S.in.quals[t.base_off + ((t.bits & 1) ? t.l_seq - 1 - i : i)] - 33); }
	int k = off - t.o_aux;
	if (t.rgl > 0) {
		if (k < 3) return (uint32_t)"RGZ"[k];
		k -= 3;
		if (k <= t.rgl) return k == t.rgl ? 0u : S.in.rgs[S.in.rg_off[p] + k];
		k -= t.rgl + 1;
	}
	if (k < REC_FIXED_AUX) {
		if (k < 3) return (uint32_t)"ASi"[k];
		if (k < 7) return ((uint32_t)t.score >> (8 * (k - 3))) & 0xffu;
		if (k < 12) return (uint32_t)(uint8_t)"XMZ0"[k - 7];                  // (the literal's own NUL ends the string)
		if (k < 17) return k == 15 ? ((t.bits & 2) ? (uint32_t)'1' : (uint32_t)'0') : (uint32_t)(uint8_t)"AMZ\0"[k - 12];
		return (uint32_t)(uint8_t)"XTC"[k - 17];
	}
	k -= REC_FIXED_AUX; // BX:Z + VX:C:1 (only a record with bit 4 is that long)
	if (k < 3) return (uint32_t)"BXZ"[k];
	k -= 3;
	if (k <= t.bcl) return k == t.bcl ? 0u : S.in.barcodes[S.in.barcode_off[t.set] + k];
	k -= t.bcl + 1;
	return k < 3 ? (uint32_t)"VXC"[k] : 1u;
}

// The fill, output-stationary: lane w owns stream bytes [16 w, 16 w + 16), computes each of them from (record, offset within the record) and
// issues ONE aligned 16-byte store -- neighbouring lanes write neighbouring words (a wavefront's store instruction covers 1 KiB in one piece),
// no stream byte is written twice, nothing depends on lane order.  16 rather than 4 bytes per lane: it is the widest store there is, and the
// search for the word's record (tile table, then a walk of at most 7 records: a record is at least 40 bytes, a tile 256) and the load of its
// RecMeta are paid once per 16 bytes instead of once per 4.  A record is longer than a word, so a word meets at most one record boundary.
// Bytes of the last word past the end of the stream are zero.
struct KBamRecFill {
	RecSources S; const RecMeta *meta; const int32_t *rec_off, *tile_first; int n_rec; int64_t total; RecWord16 *out;
	ARX_DEV void operator()(int w, int) const
	{
		const int64_t b0 = (int64_t)w * 16;
		int r = tile_first[w / (REC_TILE / 16)];
		while (r + 1 < n_rec && (int64_t)rec_off[r + 1] <= b0) ++r;
		const RecMeta *t = meta + r; // (read where it lies: a copy in registers would be indexed by the offset and go to scratch)
		int off = (int)(b0 - rec_off[r]);
		RecWord16 v;
		v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
#pragma unroll
		for (int k = 0; k < 16 && b0 + k < total; ++k) {
			if (off == t->size) { ++r; ++t; off = 0; } // (b0 + k < total: record r + 1 exists)
			v.w[k >> 2] |= rec_byte(S, *t, r, off) << (8 * (k & 3));
			++off;
		}
		out[w] = v;
	}
};

} // namespace arx

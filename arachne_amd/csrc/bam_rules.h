// bam_rules.h -- the rules that turn a placed candidate into the fields of a BAM record, stated once for everything that builds records: the
// host builder (bam_records.h, both modes), the host encoder (bam_sink.h) and the device functors (dev_records.h).  Needs <stdint.h> and
// arx_hd.h alone, so host-compiled and HIP code include it alike; the functions that read a candidate are templates over its type (arx_cand
// of the C ABI and the device's Cand are layout twins).  Citations: src/aligner/bamwriter.go unless a file is named.
#pragma once
#include <stdint.h>
#include "arx_hd.h"

namespace arx {

// IsUnmapped (aligner.go:140-145), the score rule: AppendBam applies it to the record's own candidate (:287-290), to the mate's score under
// the PRIMARY's is_proper (mate unmapped, TempLen), and to a split candidate under arx_split's is_proper
ARX_HDI bool bam_score_rule(bool is_proper, int score) { return !is_proper && score - 17 < 19; }
template <class C> ARX_HDI bool bam_score_rule(const C &a) { return bam_score_rule(a.is_proper != 0, a.score); }
// ... and what a record is written as: the placeholder of a read without hits (pos -1) is unmapped too
template <class C> ARX_HDI bool bam_unmapped(const C &a) { return a.pos == -1 || bam_score_rule(a); }

// the candidate DoDumpToBam writes as `primary` (:635-658): the LAST one of read r with `active` set, -1 if there is none
template <class C> ARX_HDI int bam_active(const C *cands, const int32_t *cand_off, int64_t r)
{
	int a = -1;
	for (int i = cand_off[r]; i < cand_off[r + 1]; ++i) if (cands[i].active) a = i;
	return a;
}

// flag word (:286-366): paired always; mate reversed only on a record whose mate is mapped
ARX_HDI uint32_t bam_flag(bool second, bool proper, bool unmapped, bool mate_unmapped, bool mate_reversed, bool reversed, bool duplicate, bool secondary)
{
	uint32_t fl = 0x1u | (second ? 0x80u : 0x40u);
	if (proper) fl |= 0x2;
	if (mate_unmapped) fl |= 0x8; else if (mate_reversed) fl |= 0x20;
	if (duplicate) fl |= 0x400;
	if (unmapped) fl |= 0x4;
	if (reversed) fl |= 0x10;
	if (secondary) fl |= 0x100;
	return fl;
}
// TempLen (:329-343) of candidate c with mate m, from their positions AS WRITTEN (the full mode passes them after AppendBam's mutation).
// Reverse-strand candidates carry the swapped pos / aend of aligner.go:1577-1582, so this reads the fields the reference reads
template <class C> ARX_HDI int32_t bam_tlen(const C &c, const C &m, int64_t cpos, int64_t mpos)
{
	if (mpos == -1 || c.rid != m.rid || bam_score_rule(c.is_proper, m.score)) return 0;
	return c.reversed ? -(int32_t)(c.aend - mpos) : (int32_t)(m.aend - cpos);
}
ARX_HDI uint32_t bam_mapq(int32_t q) { return (uint32_t)(q < 0 ? 0 : (q > 255 ? 255 : q)); } // the MAPQ byte

// a CIGAR word with BWA's op (MIDSH = 0..4) as BAM's (M I D S H = 0 1 2 4 5): fixCigar's table (:248-276)
ARX_HDI uint32_t bam_cigar_word(uint32_t w) { const uint32_t op = w & 15u; return (w & ~15u) | (op < 5 ? (0x54210u >> (4 * op)) & 15u : op); }
// reference bases n CIGAR words cover (BAM ops M D N = X: 0, 2, 3, 7, 8); bwa_ops: the words still carry BWA's ops
ARX_HDI int64_t bam_ref_len(const uint32_t *cig, int n, bool bwa_ops)
{
	int64_t len = 0;
	for (int k = 0; k < n; ++k) { const uint32_t w = bwa_ops ? bam_cigar_word(cig[k]) : cig[k], op = w & 15u; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) len += w >> 4; }
	return len;
}
// reg2bin (SAM specification 5.3): the bin of [beg, end)
ARX_HDI int reg2bin(int64_t beg, int64_t end)
{
	--end;
	if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
	return 0;
}
// bin of a record at pos covering ref_len bases; unmapped: reg2bin(-1, 0)
ARX_HDI int bam_bin(int32_t pos, int64_t ref_len) { return pos < 0 ? 4680 : reg2bin(pos, (int64_t)pos + (ref_len > 0 ? ref_len : 1)); }

// which sets carry BX / VX: attach_bx = unique_barcode (aligner.go:474, 499) and a '-' in the barcode (:389, 555)
ARX_HDI bool bam_set_bx(bool unique, const char *barcode, int64_t len)
{
	for (int64_t i = 0; i < len; ++i) if (barcode[i] == '-') return unique;
	return false;
}
// aux bytes of arx_recbuf_build's record: RG:Z (only a non-empty read group of rgl bytes), the fixed tags, BX:Z (bcl bytes) + VX:C:1 (:555-559)
constexpr int REC_FIXED_AUX = 21; // AS:i as int32 (7) XM:Z:0 (5) AM:Z:x (5) XT:C:0 (4)
template <class I> ARX_HDI I bam_first_aux_len(I rgl, bool bx, I bcl) { return (rgl > 0 ? 3 + rgl + 1 : 0) + REC_FIXED_AUX + (bx ? 3 + bcl + 1 + 4 : 0); }

// the 36-byte fixed part as nine little-endian words: block_size (the record's size minus this field), refID, pos, l_read_name | mapq << 8 |
// bin << 16, n_cigar_op | flag << 16, l_seq, next_refID, next_pos, tlen.  l_name counts the NUL; callers keep it, mapq and n_cig in their fields
ARX_HDI void bam_fixed(uint32_t *f, int64_t size, int32_t rid, int32_t pos, uint32_t l_name, uint32_t mapq, int bin, uint32_t n_cig, uint32_t flag, uint32_t l_seq,
                       int32_t mate_rid, int32_t mate_pos, int32_t tlen)
{
	f[0] = (uint32_t)(size - 4); f[1] = (uint32_t)rid; f[2] = (uint32_t)pos;
	f[3] = l_name | mapq << 8 | (uint32_t)bin << 16;
	f[4] = (n_cig & 0xffffu) | flag << 16;
	f[5] = l_seq; f[6] = (uint32_t)mate_rid; f[7] = (uint32_t)mate_pos; f[8] = (uint32_t)tlen;
}

// ---- the full record set (arx_recbuf_build_full, arx_batch_records_full): what AppendBam decides for a read's primary and split record

// isPair (aligner.go:1032) on positions as mutated
template <class C> ARX_HDI bool bam_pair_at(const C &a, int64_t apos, const C &b, int64_t bpos)
{
	if (a.reversed == b.reversed || a.rid != b.rid) return false;
	const int64_t dist = a.reversed ? apos - bpos : bpos - apos;
	return dist >= -35 && dist < 750;
}
// What AppendBam sees when it writes read r's records: the mutation of the score rule applied in write order (:286-366)
struct BamReadState {
	int a, am, s;          // active candidate, the mate's, the split candidate (-1: none)
	int64_t cpos, mpos;    // the primary's pos as written; the mate's pos when r's records are written (2p+1 sees 2p's mutation)
	bool mate_un;          // flag 0x8 of both records
	int64_t spos;          // the split record's pos as written
	int hc0, hc1;          // HardClip (:660-689): bases cut at the front / the back of the split record
};
// a / am: the active candidates of read r and of its mate; sp: the read's arx_split / SplitRec
template <class C, class A, class S> ARX_HDI BamReadState bam_read_state(const C *cands, const A *alns, const uint32_t *cigs, int a, int am, const S &sp, int64_t r)
{
	BamReadState st;
	st.a = a; st.am = am; st.s = sp.split;
	const C &c = cands[a], &m = cands[am];
	st.cpos = bam_score_rule(c) ? -1 : c.pos;
	st.mpos = ((r & 1) && bam_score_rule(m)) ? -1 : m.pos;
	st.mate_un = st.mpos == -1 || bam_score_rule(c.is_proper != 0, m.score);
	st.spos = -1; st.hc0 = st.hc1 = 0;
	if (st.s >= 0) {
		const C &x = cands[st.s];
		st.spos = bam_score_rule(sp.is_proper != 0, x.score) ? -1 : x.pos;
		const A &al = alns[x.reg];
		const uint32_t *w = cigs + al.cigar_off;
		if (al.n_cigar >= 1 && (w[0] & 15u) == 3) st.hc0 = (int)(w[0] >> 4);                                  // BWA's S = 3 (BAM's 4)
		if (al.n_cigar >= 2 && (w[al.n_cigar - 1] & 15u) == 3) st.hc1 = (int)(w[al.n_cigar - 1] >> 4);
	}
	return st;
}
// arx_split may only name a candidate of its own read that has an alignment; the text of every check that refuses another
template <class C> ARX_HDI bool bam_split_ok(const C *cands, const int32_t *cand_off, int64_t r, int sp) { return sp < 0 || (sp >= cand_off[r] && sp < cand_off[r + 1] && cands[sp].reg >= 0); }
#define ARX_BAM_SPLIT_TEXT "arx_split names a candidate of another read"
// flag word of the split record x of a read whose mate is m: secondary, proper only if arx_split says so AND the positions as written pair
template <class C> ARX_HDI uint32_t bam_split_flag(bool second, bool sp_is_proper, const C &x, const BamReadState &st, const C &m, bool duplicate)
{
	return bam_flag(second, sp_is_proper && bam_pair_at(x, st.spos, m, st.mpos), st.spos == -1, st.mate_un, m.reversed, x.reversed, duplicate, true);
}
// the fields of a record of candidate x written at xpos (-1: unmapped) with MAPQ mq, its mate m at mpos
struct BamFields { int32_t rid, pos, mate_rid, mate_pos; uint32_t mapq; };
template <class C> ARX_HDI BamFields bam_fields(const C &x, int64_t xpos, int32_t mq, bool mate_un, const C &m, int64_t mpos)
{
	BamFields f;
	f.rid = xpos == -1 ? -1 : x.rid; f.pos = (int32_t)xpos; f.mapq = xpos == -1 ? 0u : bam_mapq(mq);
	f.mate_rid = mate_un ? -1 : m.rid; f.mate_pos = mate_un ? -1 : (int32_t)mpos;
	return f;
}
// a split record's CIGAR word k of n (already BAM's ops): S at either end becomes H (HardClip, :660-689)
ARX_HDI uint32_t bam_hard_word(uint32_t w, int k, int n) { return ((k == 0 || (k == n - 1 && n >= 2)) && (w & 15u) == 4) ? (w & ~15u) | 5u : w; }
// the position bucket (:280, arx_bucket_table): the unmapped file for a record the score rule unmaps (the primary: of its own candidate; the
// split record: under arx_split's is_proper, i.e. spos == -1), else the chunk of the candidate's own pos.  (A contig outside the table can
// only be the placeholder's -1, which the score rule unmaps.)
ARX_HDI int32_t bam_bucket(bool unmapped, int32_t rid, int64_t pos, const int32_t *contig_file, int32_t n_contigs, int64_t chunk, int32_t unmapped_file)
{
	return (unmapped || rid < 0 || rid >= n_contigs) ? unmapped_file : contig_file[rid] + (int32_t)(pos / chunk);
}
// The aux fields in the reference's order (:390-563) and the bytes each takes.  Integers are `i` (7 bytes), strings tag + 'Z' + text + NUL
enum { FA_RG, FA_XS, FA_XC, FA_AC, FA_AS, FA_XM, FA_AM, FA_XT, FA_SA, FA_BX, FA_VX, FA_DM, FA_N };
struct BamFullAux { int32_t rgl, l_xc, l_ac, l_sa, bcl, l_dm; bool bx; }; // text bytes; rgl 0: no RG; l_sa / l_dm < 0: no SA / DM; bx: BX + VX
ARX_HDI int32_t bam_full_field_len(const BamFullAux &a, int f)
{
	switch (f) {
	case FA_RG: return a.rgl > 0 ? 4 + a.rgl : 0;
	case FA_XC: return 4 + a.l_xc;
	case FA_AC: return 4 + a.l_ac;
	case FA_XM: case FA_AM: return 5;
	case FA_SA: return a.l_sa >= 0 ? 4 + a.l_sa : 0;
	case FA_BX: return a.bx ? 4 + a.bcl : 0;
	case FA_VX: return a.bx ? 7 : 0;
	case FA_DM: return a.l_dm >= 0 ? 4 + a.l_dm : 0;
	default: return 7; // XS AS XT
	}
}
ARX_HDI int32_t bam_full_aux_len(const BamFullAux &a) { int32_t n = 0; for (int f = 0; f < FA_N; ++f) n += bam_full_field_len(a, f); return n; }
// XS / AS / XT / XM of a record: arx_batch_tags' for the primary; the split's halves, truncated toward zero as C divides, XT 0, XM 0
template <class T, class S> ARX_HDI void bam_full_ints(bool split, const T &t, const S &sp, int32_t *xs, int32_t *as, int32_t *xt, bool *xm)
{
	*xs = split ? sp.second_best2 / 2 : t.xs; *as = split ? sp.score2 / 2 : t.as; *xt = split ? 0 : t.xt; *xm = !split && t.xm;
}
// SA (:462-494): the primary points at its split candidate, written BEFORE the split record's own mutation (the candidate's pos, arx_split's
// MAPQ, S printed as H, :478-480); the split record points at the primary as written, and has no SA when the primary was unmapped
ARX_HDI bool bam_has_sa(bool split, const BamReadState &st) { return split ? st.cpos > -1 : st.s >= 0; }
template <class C, class S> ARX_HDI void bam_sa_source(bool split, const BamReadState &st, const C *cands, const S &sp, int *cand, int64_t *pos, int32_t *mapq, bool *hard)
{
	if (split) { *cand = st.a; *pos = st.cpos; *mapq = cands[st.a].mapq; *hard = false; }
	else { *cand = st.s; *pos = cands[st.s].pos; *mapq = sp.mapq; *hard = true; }
}
// its CIGAR text: the raw BWA words, in reversed order for a reverse-strand candidate; NM = mismatch locations + I/D lengths
ARX_HDI uint32_t bam_sa_word(const uint32_t *cig, int n, int k, bool reversed) { return cig[reversed ? n - 1 - k : k]; }
ARX_HDI char bam_sa_op(uint32_t w, bool hard) { const uint32_t op = w & 15u; return op == 3 ? (hard ? 'H' : 'S') : "MIDSH"[op < 5 ? op : 4]; }
ARX_HDI int32_t bam_sa_nm(int32_t n_mm, const uint32_t *cig, int n)
{
	int32_t indel = 0;
	for (int k = 0; k < n; ++k) { const uint32_t op = cig[k] & 15u; if (op == 1 || op == 2) indel += (int32_t)(cig[k] >> 4); }
	return n_mm + indel;
}
// DM (:560-563): primary records of a set with BX whose candidate is in the active molecule, when the molecule has active alignments
ARX_HDI bool bam_has_dm(bool split, bool bx, bool active_molecule, int32_t dm_n) { return bx && !split && active_molecule && dm_n > 0; }

// a read name is 1..254 bytes (l_read_name is one byte and counts the NUL); the text of every check that refuses one (a std::string expression)
ARX_HDI bool bam_name_ok(int64_t len) { return len >= 1 && len <= 254; }
#define ARX_BAM_NAME_TEXT(record) ("read name of record " + std::to_string(record) + " must be 1..254 bytes")

} // namespace arx

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

// a read name is 1..254 bytes (l_read_name is one byte and counts the NUL); the text of every check that refuses one (a std::string expression)
ARX_HDI bool bam_name_ok(int64_t len) { return len >= 1 && len <= 254; }
#define ARX_BAM_NAME_TEXT(record) ("read name of record " + std::to_string(record) + " must be 1..254 bytes")

} // namespace arx

// dev_records_full.h -- the reference's record set encoded on the device (arx_batch_records_full): what RecBuf::build's FULL mode
// (bam_records.h) followed by BamSink::encode (bam_sink.h) writes -- every read's primary record, its split record behind it, the tags RG XS
// XC AC AS XM AM XT SA BX VX DM, the position bucket of every record -- and the same records a second time, grouped by bucket (AppendBams
// writes every record twice, bamwriter.go:279-281).  What a read's records ARE is bam_rules.h's (BamReadState, the split record's flag and
// fields, order and length of the aux fields, SA's source / word order / H-for-S / NM, the bucket), shared with the host builder; what is stated
// here is where each byte comes from (rec_full_part / rec_full_byte) and the decimal text the host gets from snprintf.  Compiled for the
// device and for the host test doubles.
//
// Launch order (pipeline_records.h, RecordsFullStage), every functor through launch_wide:
//   KRecMmLen      one mismatch entry per lane: bytes of its "%d,%d,1;"                         -> scan -> mm_txt_off
//   KRecFullCount  one read per lane: 1 record, or 2 with a split; the error bits               -> scan -> rbase (the read's first record)
//   KRecFullMeta   one read per lane: RecFullMeta, size and bucket of its records               -> scan -> rec_off
//   KBamRecTile, KRecFullFill     the stream, as dev_records.h's: one aligned 16-byte store per lane, every byte a function of (record, offset)
//   KRecGroupCount / KRecGroupRank / KRecGroupSize / KRecGroupOff   the stable order by bucket (see there), the grouped records' sizes -> scan,
//                  the two offset tables; then KBamRecTile and KRecFullFill again over the permuted order: nothing is encoded twice over
#pragma once
#include <math.h>
#include "dev_records.h"

namespace arx {

enum : uint32_t { REC_ERR_SPLIT = 2, REC_ERR_BUCKET = 4 };  // (REC_ERR_NO_ACTIVE = 1)
constexpr int REC_GROUP_BLOCK = 256;    // records per block of the grouping
constexpr int REC_MAX_FILES = 4096;     // buckets the grouping table is sized for (n_files * blocks entries, see KRecGroupCount)
constexpr int64_t REC_MAX_GROUP_TABLE = (int64_t)1 << 26; // entries of that table a call accepts: it is held twice as int32 (2 x 256 MiB), zeroed twice and scanned once

// ---- decimal text: what snprintf("%d") / ("%lld") / ("%.6f") writes, as (length, character i) so that a lane can write any byte of it
ARX_HDI int dec_len32(uint32_t v)
{
	return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}
ARX_HDI uint32_t dec_digit32(uint32_t v, int nd, int i) // digit i (from the left) of v written with nd digits: a division by a constant
{
	switch (nd - 1 - i) {
	case 0: return v % 10u;
	case 1: return v / 10u % 10u;
	case 2: return v / 100u % 10u;
	case 3: return v / 1000u % 10u;
	case 4: return v / 10000u % 10u;
	case 5: return v / 100000u % 10u;
	case 6: return v / 1000000u % 10u;
	case 7: return v / 10000000u % 10u;
	case 8: return v / 100000000u % 10u;
	default: return v / 1000000000u % 10u;
	}
}
ARX_HDI int dec_len64(uint64_t v) { if (v <= 0xffffffffull) return dec_len32((uint32_t)v); int n = 1; while (v >= 10) { v /= 10; ++n; } return n; }
ARX_HDI uint32_t dec_digit64(uint64_t v, int nd, int i)
{
	if (v <= 0xffffffffull) return dec_digit32((uint32_t)v, nd, i);
	for (int k = nd - 1 - i; k > 0; --k) v /= 10;
	return (uint32_t)(v % 10);
}
ARX_HDI int int_len(int32_t v) { return v < 0 ? 1 + dec_len32(0u - (uint32_t)v) : dec_len32((uint32_t)v); } // "%d" (INT32_MIN included)
ARX_HDI uint32_t int_char(int32_t v, int i)
{
	if (v >= 0) return '0' + dec_digit32((uint32_t)v, dec_len32((uint32_t)v), i);
	const uint32_t m = 0u - (uint32_t)v;
	return i == 0 ? (uint32_t)'-' : '0' + dec_digit32(m, dec_len32(m), i - 1);
}
ARX_HDI int int64_len(int64_t v) { return v < 0 ? 1 + dec_len64(0ull - (uint64_t)v) : dec_len64((uint64_t)v); } // "%lld"
ARX_HDI uint32_t int64_char(int64_t v, int i)
{
	if (v >= 0) return '0' + dec_digit64((uint64_t)v, dec_len64((uint64_t)v), i);
	const uint64_t m = 0ull - (uint64_t)v;
	return i == 0 ? (uint32_t)'-' : '0' + dec_digit64(m, dec_len64(m), i - 1);
}
// DM: snprintf("%.6f", (double)s / (double)n) for 0 <= s < 2^31, 0 < n < 2^31, as the integer t it prints (t / 10^6 '.' t % 10^6).  printf
// converts the double q = fl(s / n) exactly and rounds half to even, so t is round(q * 10^6); the exact quotient x = s / n lies within
// x * 2^-53 of q.  Off a tie the exact x * 10^6 is at least 1 / (2 n) away from the rounding boundary t + 1/2 (2 rem - n is a non-zero
// integer), i.e. x is at least 1 / (2 n 10^6) from it, while |q - x| <= (s / n) * 2^-53 < 2^31 * 2^-53 / n = 2^-22 / n < 2.4e-7 / n, below
// 5e-7 / n: q and x round alike, and integer arithmetic on x decides.  On a tie (2 rem == n) x IS the boundary, and what printf sees is on
// which side q fell: d = fma(q, n, -s) is the exact sign of q * n - s (one rounding, of a value whose sign survives it).  d == 0: q is the
// tie itself, round half to even.  (Checked against snprintf on every n <= 512 with s <= 4 n, on all 220,160 ties with n = 128, 256, ..
// 32,768 and s <= 4 n -- 154,624 of them not representable in binary -- and on random pairs by tests/recsim/rec_full_sim.cpp.)
ARX_HDI uint64_t dm_scaled(uint32_t s, uint32_t n)
{
	const uint64_t a = (uint64_t)s * 1000000ull;
	uint64_t t = a / n;
	const uint64_t rem2 = 2 * (a % n);
	if (rem2 > n) return t + 1;
	if (rem2 < n) return t;
	const double q = (double)s / (double)n, d = fma(q, (double)n, -(double)s);
	if (d > 0 || (d == 0 && (t & 1))) ++t;
	return t;
}
// the text of s / n (n > 0; a negative s prints its sign, also in front of a zero as printf does)
ARX_HDI int dm_len(int32_t s, uint64_t t) { return (s < 0 ? 1 : 0) + dec_len32((uint32_t)(t / 1000000ull)) + 7; }
ARX_HDI uint32_t dm_char(bool neg, uint64_t t, int i)
{
	if (neg) { if (i == 0) return '-'; --i; }
	const uint32_t ip = (uint32_t)(t / 1000000ull), fp = (uint32_t)(t % 1000000ull);
	const int nd = dec_len32(ip);
	if (i < nd) return '0' + dec_digit32(ip, nd, i);
	return i == nd ? (uint32_t)'.' : '0' + dec_digit32(fp, 6, i - nd - 1);
}
ARX_HDI uint64_t dm_scaled_signed(int32_t s, int32_t n) { return dm_scaled(s < 0 ? 0u - (uint32_t)s : (uint32_t)s, (uint32_t)n); } // (IEEE division and fma mirror with the sign)
// one mismatch location "%d,%d,1;"
ARX_HDI int mm_entry_len(int32_t a, int32_t b) { return int_len(a) + int_len(b) + 4; }
ARX_HDI uint32_t mm_entry_char(int32_t a, int32_t b, int j)
{
	const int la = int_len(a);
	if (j < la) return int_char(a, j);
	if (j == la) return ',';
	j -= la + 1;
	const int lb = int_len(b);
	return j < lb ? int_char(b, j) : (uint32_t)",1;"[j - lb];
}

struct KRecMmLen {
	const int32_t *mm_ref, *mm_read; int32_t *len;
	ARX_DEV void operator()(int e, int) const { len[e] = mm_entry_len(mm_ref[e], mm_read[e]); }
};

// what the full record set reads beside RecInputs: arx_batch_post's and arx_batch_tags' results, the contig names (uploaded once per
// context) and the bucket table of the call
struct RecFullInputs {
	const CandPost *post; const SplitRec *split; const ReadTags *tags;
	const int32_t *mm_ref, *mm_read, *mm_txt_off;         // mm_txt_off[e]: where entry e's text starts in the text of all entries (n_mm + 1)
	const uint8_t *contig_names; const int32_t *contig_name_off; // n_contigs + 1
	const int32_t *contig_file; int32_t n_contigs, unmapped_file; int64_t chunk;
};

// per record: everything the fill needs, found once
struct RecFullMeta {
	int64_t sa_pos; uint64_t dm_t;    // SA's position as written; DM as dm_scaled
	uint32_t fixed[9];
	int32_t size, o_cig, o_seq, o_qual, o_aux; // as RecMeta
	int32_t read, cig_src, n_cig, l_seq, seq0, L, base_off; // l_seq bases from base seq0 of the read as oriented (L bases): HardClip cuts the split record
	int32_t bits;                     // 1 reverse strand, 2 active molecule, 4 BX / VX, 8 split record (H at the CIGAR's ends), 16 XM, 32 SA prints S as H, 64 SA's candidate reversed, 128 DM negative
	int32_t set, rgl, bcl;
	int32_t xs, as, xt;
	int32_t l_xc, xc_mm0, xc_n, l_ac, ac_mm0, ac_n; // text bytes, first entry and entries of the mismatch list behind XC / AC
	int32_t l_sa, sa_rid, sa_cig_src, sa_n_cig, sa_l_cig, sa_mapq, sa_nm; // l_sa < 0: no SA; sa_rid < 0: empty contig name
	int32_t l_dm;                     // < 0: no DM
	int32_t pad[2];
};
static_assert(sizeof(RecFullMeta) == 192, "RecFullMeta is twelve 16-byte words");
ARX_HDI BamFullAux rec_full_aux(const RecFullMeta &t) { return BamFullAux{t.rgl, t.l_xc, t.l_ac, t.l_sa, t.bcl, t.l_dm, (t.bits & 4) != 0}; }

struct KRecFullCount {
	const Cand *cands; const int32_t *cand_off; const SplitRec *split; int32_t *n_rec; uint32_t *err;
	ARX_DEV void operator()(int r, int) const
	{
		if (bam_active(cands, cand_off, r) < 0) ARX_ATOMIC_OR(err, REC_ERR_NO_ACTIVE);
		const int sp = split[r].split;
		if (!bam_split_ok(cands, cand_off, r, sp)) ARX_ATOMIC_OR(err, REC_ERR_SPLIT);
		n_rec[r] = sp >= 0 ? 2 : 1;
	}
};

// Runs only on a batch KRecFullCount found no fault with: every read has an active candidate, every split candidate an alignment
struct KRecFullMeta {
	const Cand *cands; const int32_t *cand_off; const Aln *alns; const uint32_t *cig;
	const int32_t *lens, *base_off; RecInputs in; RecFullInputs F; const int32_t *rbase;
	RecFullMeta *meta; int32_t *size, *bucket; uint32_t *err;
	ARX_DEV int mm_text(int c, int32_t *mm0, int32_t *n) const // bytes of candidate c's list (c < 0: none)
	{
		*mm0 = 0; *n = 0;
		if (c < 0) return 0;
		*mm0 = F.post[c].mm_off; *n = F.post[c].n_mm;
		return F.mm_txt_off[*mm0 + *n] - F.mm_txt_off[*mm0];
	}
	ARX_DEV void record(int r, int q, bool split, const BamReadState &st, int s, int rgl, int bcl, bool bx, int l_name) const
	{
		const int xi = split ? st.s : st.a;
		const Cand &x = cands[xi], &m = cands[st.am];
		const SplitRec &S = F.split[r]; const ReadTags &T = F.tags[r];
		const bool dup = F.post[xi].duplicate != 0;
		const uint32_t fl = split ? bam_split_flag(r & 1, S.is_proper != 0, x, st, m, dup) : bam_flag(r & 1, x.is_proper, st.cpos == -1, st.mate_un, m.reversed, x.reversed, dup, false);
		const BamFields f = bam_fields(x, split ? st.spos : st.cpos, split ? S.mapq : x.mapq, st.mate_un, m, st.mpos);
		const int32_t tl = split ? 0 : bam_tlen(x, m, st.cpos, st.mpos);
		const int n_cig = x.reg >= 0 ? alns[x.reg].n_cigar : 0, cig_src = x.reg >= 0 ? alns[x.reg].cigar_off : 0;
		const int bin = bam_bin(f.pos, bam_ref_len(cig + cig_src, n_cig, true)); // (H for S at the ends covers no reference base either)
		const int L = lens[r], kept = split ? (L - st.hc0 - st.hc1 > 0 ? L - st.hc0 - st.hc1 : 0) : L;
		RecFullMeta t;
		t.read = r; t.cig_src = cig_src; t.n_cig = n_cig; t.l_seq = kept; t.seq0 = split ? st.hc0 : 0; t.L = L; t.base_off = base_off[r];
		t.set = s; t.rgl = rgl; t.bcl = bcl;
		bool xm;
		bam_full_ints(split, T, S, &t.xs, &t.as, &t.xt, &xm);
		t.bits = (x.reversed ? 1 : 0) | (x.active_molecule ? 2 : 0) | (bx ? 4 : 0) | (split ? 8 : 0) | (xm ? 16 : 0);
		t.l_xc = mm_text(split ? -1 : T.second_best, &t.xc_mm0, &t.xc_n);
		t.l_ac = mm_text(xi, &t.ac_mm0, &t.ac_n);
		t.l_sa = -1; t.sa_pos = 0; t.sa_rid = -1; t.sa_cig_src = t.sa_n_cig = t.sa_l_cig = t.sa_mapq = t.sa_nm = 0;
		if (bam_has_sa(split, st)) {
			int i; bool hard;
			bam_sa_source(split, st, cands, S, &i, &t.sa_pos, &t.sa_mapq, &hard);
			const Cand &y = cands[i];
			if (y.reg >= 0) { t.sa_cig_src = alns[y.reg].cigar_off; t.sa_n_cig = alns[y.reg].n_cigar; }
			for (int k = 0; k < t.sa_n_cig; ++k) t.sa_l_cig += dec_len32(cig[t.sa_cig_src + k] >> 4) + 1;
			t.sa_nm = bam_sa_nm(F.post[i].n_mm, cig + t.sa_cig_src, t.sa_n_cig);
			t.sa_rid = (y.rid >= 0 && y.rid < F.n_contigs) ? y.rid : -1;
			const int nl = t.sa_rid >= 0 ? F.contig_name_off[t.sa_rid + 1] - F.contig_name_off[t.sa_rid] : 0;
			t.l_sa = nl + int64_len(t.sa_pos) + t.sa_l_cig + int_len(t.sa_mapq) + int_len(t.sa_nm) + 7; // five commas, the strand, ';'
			t.bits |= (hard ? 32 : 0) | (y.reversed ? 64 : 0);
		}
		t.l_dm = -1; t.dm_t = 0;
		if (bam_has_dm(split, bx, x.active_molecule != 0, T.dm_n)) {
			t.dm_t = dm_scaled_signed(T.dm_sum, T.dm_n);
			t.l_dm = dm_len(T.dm_sum, t.dm_t);
			if (T.dm_sum < 0) t.bits |= 128;
		}
		t.o_cig = 36 + l_name; t.o_seq = t.o_cig + 4 * n_cig; t.o_qual = t.o_seq + (kept + 1) / 2; t.o_aux = t.o_qual + kept;
		t.size = t.o_aux + bam_full_aux_len(rec_full_aux(t));
		bam_fixed(t.fixed, t.size, f.rid, f.pos, (uint32_t)l_name, f.mapq, bin, (uint32_t)n_cig, fl, (uint32_t)kept, f.mate_rid, f.mate_pos, tl);
		t.pad[0] = t.pad[1] = 0;
		meta[q] = t; size[q] = t.size;
		int32_t bk = split ? bam_bucket(st.spos == -1, x.rid, x.pos, F.contig_file, F.n_contigs, F.chunk, F.unmapped_file)
		                   : bam_bucket(bam_score_rule(x), x.rid, x.pos, F.contig_file, F.n_contigs, F.chunk, F.unmapped_file);
		if (bk < 0 || bk > F.unmapped_file) { ARX_ATOMIC_OR(err, REC_ERR_BUCKET); bk = F.unmapped_file; } // (the grouping indexes its table by it)
		bucket[q] = bk;
	}
	ARX_DEV void operator()(int r, int) const
	{
		const int a = bam_active(cands, cand_off, r), am = bam_active(cands, cand_off, r ^ 1);
		const BamReadState st = bam_read_state(cands, alns, cig, a, am, F.split[r], r);
		const int p = r >> 1;
		int lo = 0, hi = in.n_sets; // the set of pair p: the last one that starts at or before it
		while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (in.set_pair_off[mid] <= p) lo = mid; else hi = mid; }
		const int s = lo;
		const int l_name = (int)(in.name_off[p + 1] - in.name_off[p]) + 1;
		const int rgl = (int)(in.rg_off[p + 1] - in.rg_off[p]), bcl = (int)(in.barcode_off[s + 1] - in.barcode_off[s]);
		const bool bx = in.set_bx[s] != 0;
		const int q = rbase[r];
		record(r, q, false, st, s, rgl, bcl, bx, l_name);
		if (st.s >= 0) record(r, q + 1, true, st, s, rgl, bcl, bx, l_name);
	}
};

// ---- the bytes.  A record is a sequence of parts: the fixed part, name, CIGAR, bases, qualities, then the aux fields in bam_rules.h's order
enum { RP_FIXED, RP_NAME, RP_CIG, RP_SEQ, RP_QUAL, RP_AUX }; // RP_AUX + FA_*
struct RecFullSources { const uint32_t *cig; const uint8_t *bases; RecInputs in; RecFullInputs F; };
// the part byte `off` of the record lies in, and where the part starts and ends: what the fill resolves once and steps from
struct RecPart { int part, lo, hi; };
ARX_DEVI RecPart rec_full_part(const RecFullMeta &t, int off)
{
	if (off < 36) return RecPart{RP_FIXED, 0, 36};
	if (off < t.o_cig) return RecPart{RP_NAME, 36, t.o_cig};
	if (off < t.o_seq) return RecPart{RP_CIG, t.o_cig, t.o_seq};
	if (off < t.o_qual) return RecPart{RP_SEQ, t.o_seq, t.o_qual};
	if (off < t.o_aux) return RecPart{RP_QUAL, t.o_qual, t.o_aux};
	const BamFullAux a = rec_full_aux(t);
	int lo = t.o_aux;
	for (int f = 0; f < FA_N - 1; ++f) { const int n = bam_full_field_len(a, f); if (off < lo + n) return RecPart{RP_AUX + f, lo, lo + n}; lo += n; }
	return RecPart{RP_AUX + FA_DM, lo, t.size};
}
// the mismatch entry a lane is inside: its index and its text range in mm_txt_off's coordinates.  Consecutive bytes stay in it or step to the next
struct MmCursor { int e, t0, t1; };
ARX_DEVI uint32_t mm_list_char(const RecFullSources &S, int mm0, int n, int k, MmCursor &cu) // byte k of the text of entries [mm0, mm0 + n)
{
	const int32_t *to = S.F.mm_txt_off;
	const int tp = to[mm0] + k;
	if (tp < cu.t0 || tp >= cu.t1) {
		if (tp == cu.t1 && cu.e >= mm0 && cu.e + 1 < mm0 + n) ++cu.e;
		else { int lo = mm0, hi = mm0 + n - 1; while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (to[mid] <= tp) lo = mid; else hi = mid - 1; } cu.e = lo; } // the last entry that starts at or before tp
		cu.t0 = to[cu.e]; cu.t1 = to[cu.e + 1];
	}
	return mm_entry_char(S.F.mm_ref[cu.e], S.F.mm_read[cu.e], tp - cu.t0);
}
ARX_DEVI uint32_t sa_char(const RecFullSources &S, const RecFullMeta &t, int k) // byte k of "contig,pos,strand,cigar,mapq,NM;"
{
	if (t.sa_rid >= 0) {
		const int nl = S.F.contig_name_off[t.sa_rid + 1] - S.F.contig_name_off[t.sa_rid];
		if (k < nl) return S.F.contig_names[S.F.contig_name_off[t.sa_rid] + k];
		k -= nl;
	}
	if (k == 0) return ',';
	--k;
	const int pl = int64_len(t.sa_pos);
	if (k < pl) return int64_char(t.sa_pos, k);
	k -= pl;
	if (k < 3) return k == 1 ? ((t.bits & 64) ? (uint32_t)'-' : (uint32_t)'+') : (uint32_t)',';
	k -= 3;
	if (k < t.sa_l_cig) {
		for (int j = 0; j < t.sa_n_cig; ++j) { // (a walk over the words: their texts have no offsets of their own)
			const uint32_t w = bam_sa_word(S.cig + t.sa_cig_src, t.sa_n_cig, j, (t.bits & 64) != 0);
			const int dl = dec_len32(w >> 4);
			if (k < dl) return '0' + dec_digit32(w >> 4, dl, k);
			if (k == dl) return (uint32_t)(uint8_t)bam_sa_op(w, (t.bits & 32) != 0);
			k -= dl + 1;
		}
		return 0;
	}
	k -= t.sa_l_cig;
	if (k == 0) return ',';
	--k;
	const int ml = int_len(t.sa_mapq);
	if (k < ml) return int_char(t.sa_mapq, k);
	k -= ml;
	if (k == 0) return ',';
	--k;
	return k < int_len(t.sa_nm) ? int_char(t.sa_nm, k) : (uint32_t)';';
}
ARX_DEVI uint32_t rec_full_base4(const RecFullSources &S, const RecFullMeta &t, int i) // 4-bit code of base i of the record as written
{
	const bool rev = t.bits & 1;
	const int k = t.seq0 + i;
	const uint32_t y = S.bases[t.base_off + (rev ? t.L - 1 - k : k)];
	if (y > 3) return 15u;
	return 1u << (rev ? 3 - y : y);
}
ARX_DEVI uint32_t aux_i32(const char *tag, int32_t v, int k) { return k < 2 ? (uint32_t)(uint8_t)tag[k] : k == 2 ? (uint32_t)'i' : ((uint32_t)v >> (8 * (k - 3))) & 0xffu; }
// byte k of part `part` of the record with meta t
ARX_DEVI uint32_t rec_full_byte(const RecFullSources &S, const RecFullMeta &t, int part, int k, MmCursor &cu)
{
	const int p = t.read >> 1;
	switch (part) {
	case RP_FIXED: return (t.fixed[k >> 2] >> (8 * (k & 3))) & 0xffu;
	case RP_NAME: return k == t.o_cig - 37 ? 0u : S.in.names[S.in.name_off[p] + k];
	case RP_CIG: { uint32_t w = bam_cigar_word(S.cig[t.cig_src + (k >> 2)]); if (t.bits & 8) w = bam_hard_word(w, k >> 2, t.n_cig); return (w >> (8 * (k & 3))) & 0xffu; }
	case RP_SEQ: { const int i = 2 * k; return rec_full_base4(S, t, i) << 4 | (i + 1 < t.l_seq ? rec_full_base4(S, t, i + 1) : 0u); }
	case RP_QUAL: { const int j = t.seq0 + k; return (uint32_t)(uint8_t)(S.in.quals[t.base_off + ((t.bits & 1) ? t.L - 1 - j : j)] - 33); }
	case RP_AUX + FA_XS: return aux_i32("XS", t.xs, k);
	case RP_AUX + FA_AS: return aux_i32("AS", t.as, k);
	case RP_AUX + FA_XT: return aux_i32("XT", t.xt, k);
	case RP_AUX + FA_VX: return aux_i32("VX", 1, k);
	case RP_AUX + FA_XM: return k == 3 ? ((t.bits & 16) ? (uint32_t)'1' : (uint32_t)'0') : (uint32_t)(uint8_t)"XMZ\0"[k];
	case RP_AUX + FA_AM: return k == 3 ? ((t.bits & 2) ? (uint32_t)'1' : (uint32_t)'0') : (uint32_t)(uint8_t)"AMZ\0"[k];
	case RP_AUX + FA_RG: if (k < 3) return (uint32_t)"RGZ"[k]; k -= 3; return k == t.rgl ? 0u : S.in.rgs[S.in.rg_off[p] + k];
	case RP_AUX + FA_BX: if (k < 3) return (uint32_t)"BXZ"[k]; k -= 3; return k == t.bcl ? 0u : S.in.barcodes[S.in.barcode_off[t.set] + k];
	case RP_AUX + FA_XC: if (k < 3) return (uint32_t)"XCZ"[k]; k -= 3; return k == t.l_xc ? 0u : mm_list_char(S, t.xc_mm0, t.xc_n, k, cu);
	case RP_AUX + FA_AC: if (k < 3) return (uint32_t)"ACZ"[k]; k -= 3; return k == t.l_ac ? 0u : mm_list_char(S, t.ac_mm0, t.ac_n, k, cu);
	case RP_AUX + FA_SA: if (k < 3) return (uint32_t)"SAZ"[k]; k -= 3; return k == t.l_sa ? 0u : sa_char(S, t, k);
	default: if (k < 3) return (uint32_t)"DMZ"[k]; k -= 3; return k == t.l_dm ? 0u : dm_char((t.bits & 128) != 0, t.dm_t, k); // RP_AUX + FA_DM
	}
}

// The fill of dev_records.h over records whose parts are found by rec_full_part: lane w owns stream bytes [16 w, 16 w + 16) and issues one
// aligned 16-byte store.  The word's record comes from the tile table and a short walk, its part is resolved once and again only where the
// word crosses into the next part, the mismatch entry behind a byte of XC / AC is searched once and stepped (MmCursor).  order: null for the
// stream in record order; else stream record j is record order[j] (the grouped stream) -- rec_off and tile_first are the stream's own.
// The meta is read where it lies: a copy in registers would be indexed by the part and go to scratch
struct KRecFullFill {
	RecFullSources S; const RecFullMeta *meta; const int32_t *order; const int32_t *rec_off, *tile_first; int n_rec; int64_t total; RecWord16 *out;
	ARX_DEV void operator()(int w, int) const
	{
		const int64_t b0 = (int64_t)w * 16;
		int j = tile_first[w / (REC_TILE / 16)];
		while (j + 1 < n_rec && (int64_t)rec_off[j + 1] <= b0) ++j;
		const RecFullMeta *t = meta + (order ? order[j] : j);
		int off = (int)(b0 - rec_off[j]);
		RecPart pt = rec_full_part(*t, off);
		MmCursor cu{-1, -1, -1};
		uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0; // (four named words, chosen by compares: an array indexed by k would leave the registers unless the loop unrolls)
		for (int k = 0; k < 16 && b0 + k < total; ++k) {
			if (off == t->size) { ++j; t = meta + (order ? order[j] : j); off = 0; pt = RecPart{RP_FIXED, 0, 36}; } // (inside the stream: the next record exists)
			else if (off >= pt.hi) pt = rec_full_part(*t, off);
			const uint32_t x = rec_full_byte(S, *t, pt.part, off - pt.lo, cu) << (8 * (k & 3));
			const int h = k >> 2;
			x0 |= h == 0 ? x : 0u; x1 |= h == 1 ? x : 0u; x2 |= h == 2 ? x : 0u; x3 |= h == 3 ? x : 0u;
			++off;
		}
		RecWord16 v;
		v.w[0] = x0; v.w[1] = x1; v.w[2] = x2; v.w[3] = x3;
		out[w] = v;
	}
};

// ---- the stable order by bucket.  The records are cut into blocks of REC_GROUP_BLOCK; one lane per block counts its records per bucket into
// its own column of a bucket-major table cnt[bucket * n_blocks + block] (zeroed before), ONE exclusive scan over the table gives every block
// its base in every bucket -- all of bucket 0's blocks in order, then bucket 1's, ... -- and the same lane then ranks its records in order
// from those bases (its column of `cur`, zeroed, counts as it goes).  No atomics, no dependence on lane order; stable because blocks and
// the records inside one are both taken in order.  The table has n_files * n_blocks entries: n_files is capped at REC_MAX_FILES and the
// table at REC_MAX_GROUP_TABLE entries.  The cost of the grouping grows as n_files * n_records / REC_GROUP_BLOCK (two memsets and a scan
// over the table) and the two kernels below run ONE lane per block with serial, uncoalesced increments: built for about a hundred files
struct KRecGroupCount {
	const int32_t *bucket; int n_rec, n_blocks; int32_t *cnt;
	ARX_DEV void operator()(int b, int) const
	{
		const int lo = b * REC_GROUP_BLOCK, hi = lo + REC_GROUP_BLOCK < n_rec ? lo + REC_GROUP_BLOCK : n_rec;
		for (int q = lo; q < hi; ++q) ++cnt[(int64_t)bucket[q] * n_blocks + b];
	}
};
struct KRecGroupRank {
	const int32_t *bucket, *base; int n_rec, n_blocks; int32_t *cur, *order;
	ARX_DEV void operator()(int b, int) const
	{
		const int lo = b * REC_GROUP_BLOCK, hi = lo + REC_GROUP_BLOCK < n_rec ? lo + REC_GROUP_BLOCK : n_rec;
		for (int q = lo; q < hi; ++q) { const int64_t at = (int64_t)bucket[q] * n_blocks + b; order[base[at] + cur[at]++] = q; }
	}
};
struct KRecGroupSize { // size of the grouped stream's record j
	const int32_t *size, *order; int32_t *gsize;
	ARX_DEV void operator()(int j, int) const { gsize[j] = size[order[j]]; }
};
struct KRecGroupOff { // f = 0 .. n_files: the first record of bucket f in the grouped stream and the byte it starts at
	const int32_t *base, *g_off; int n_files, n_blocks, n_rec; int64_t *bucket_rec_off, *bucket_byte_off;
	ARX_DEV void operator()(int f, int) const
	{
		const int j = f < n_files ? base[(int64_t)f * n_blocks] : n_rec;
		bucket_rec_off[f] = j; bucket_byte_off[f] = g_off[j];
	}
};

} // namespace arx

// selftest_post.h -- arx_selftest_post (include/arachne_amd.h) for any runtime: the passes between placement and the BAM records, PostStage<RT>::run
// itself (pipeline_post.h: the CIGAR walk in its two launches around the scan, the duplicate table, the split pass), on candidates the caller made
// up.  The rows are the restatement's (oracle/arx_oracle_rfa.c: ora_post takes the same arrays).  What is filled of the batch, the work record and
// the placement result is exactly what PostStage::run and its functors read: bases, base_off, lens, n_reads; c_regs (qb, qe), c_alns (NM, n_cigar,
// cigar_off), c_cig; d_cands, n_cands, d_cand_off, d_bc_read_off, n_barcodes, penalty, d_cen_start / d_cen_end.  The index gives pac, ann_off and
// ann_len.  Included by arx_selftest.hip (HipRT) and by the host test double (tests/hostsim/sim.cpp), which compile the same pipeline_post.h.
#pragma once
#include <vector>
#include "../../include/arachne_amd.h"
#include "pipeline_post.h"

namespace arx {

constexpr int SELFTEST_POST_CAND_W = 20, SELFTEST_POST_REG_W = 20, SELFTEST_POST_ALN_W = 12; // oracle/arx_oracle.h: ORA_CAND_W, ORA_REG_W, ORA_ALN_W
constexpr int64_t SELFTEST_POST_MAX_CANDS = (int64_t)1 << 22; // a candidate lists at most one location per read base: the scan of n_mm stays inside 31 bits
constexpr int64_t SELFTEST_POST_MAX_VAL = 1 << 24;            // |score|, |lap2|, |NM|, |qb|, |qe|: the split and matches arithmetic stays far from 32 bits
constexpr int SELFTEST_POST_MAX_CIGAR = 64, SELFTEST_POST_MAX_OPLEN = 4096; // words per alignment, length of one operation (the walk loops over an M run)

// the table PostStage::run makes for R reads
inline uint32_t selftest_post_table_cap(int R) { uint32_t cap = 64; while (cap < 2u * (uint32_t)R) cap <<= 1; return cap; }

// everything a kernel would index with, checked on the host before anything is uploaded
inline bool selftest_post_args_ok(const IndexView &ix, int32_t n_reads, const int64_t *cand_off, const int64_t *cands, int64_t n_regs, const int64_t *regs, const int64_t *alns,
                                  int64_t n_cig, const int32_t *lens, int32_t n_barcodes, const int64_t *bc_pair_off)
{
	if (n_reads <= 0 || (n_reads & 1) || n_barcodes <= 0 || n_regs < 0 || n_cig < 0 || ix.n_seqs <= 0 || ix.l_pac <= 0) return false;
	if (!cand_off || !cands || !lens || !bc_pair_off || cand_off[0] != 0 || (n_regs > 0 && (!regs || !alns))) return false;
	int64_t tot = 0;
	for (int r = 0; r < n_reads; ++r) {
		if (lens[r] < 0 || lens[r] > MAX_READ_LEN) return false;
		if (cand_off[r + 1] <= cand_off[r] || cand_off[r + 1] > SELFTEST_POST_MAX_CANDS) return false; // every read has a candidate: act[r] defaults to its first
		tot += lens[r];
		for (int64_t i = cand_off[r]; i < cand_off[r + 1]; ++i) {
			const int64_t *c = cands + i * SELFTEST_POST_CAND_W;
			if (c[1] != r || c[0] < -1 || c[0] >= n_regs) return false;                  // the walk takes the read and the alignment from the row
			if (c[5] < (c[0] < 0 ? -1 : 0) || c[5] >= ix.n_seqs) return false;            // ann_off[rid], cen_start[rid]
			if (c[2] < -1 || c[3] < 0 || c[2] > 0x7fffffff || c[3] > 0x7fffffff) return false; // mm_ref holds them in 32 bits
			if (c[0] >= 0 && (c[3] < c[2] || c[3] - c[2] > SELFTEST_POST_MAX_CIGAR * (int64_t)SELFTEST_POST_MAX_OPLEN)) return false;
			if ((c[4] != 0 && c[4] != 1) || (c[12] != 0 && c[12] != 1)) return false;
			if (c[6] < -SELFTEST_POST_MAX_VAL || c[6] > SELFTEST_POST_MAX_VAL || c[11] < -SELFTEST_POST_MAX_VAL || c[11] > SELFTEST_POST_MAX_VAL) return false;
		}
	}
	if (tot >= ((int64_t)1 << 31) - 64) return false;
	for (int64_t g = 0; g < n_regs; ++g) {
		const int64_t *rg = regs + g * SELFTEST_POST_REG_W, *al = alns + g * SELFTEST_POST_ALN_W;
		if (rg[2] < -SELFTEST_POST_MAX_VAL || rg[2] > SELFTEST_POST_MAX_VAL || rg[3] < -SELFTEST_POST_MAX_VAL || rg[3] > SELFTEST_POST_MAX_VAL) return false;
		if (al[6] < -SELFTEST_POST_MAX_VAL || al[6] > SELFTEST_POST_MAX_VAL) return false;
		if (al[7] < 0 || al[7] > SELFTEST_POST_MAX_CIGAR || al[8] < 0 || al[8] + al[7] > n_cig || al[8] > 0x7fffffff) return false;
	}
	if (bc_pair_off[0] != 0 || 2 * bc_pair_off[n_barcodes] != n_reads) return false;
	for (int b = 0; b < n_barcodes; ++b) if (bc_pair_off[b + 1] <= bc_pair_off[b]) return false;
	return true;
}

struct KSelftestPostHome { // per read: the slot its key hashes to, by dup_hash itself
	const Cand *cands; const int32_t *act, *bc_of; uint32_t mask; int32_t *home;
	ARX_DEV void operator()(int r, int) const { home[r] = (int32_t)(dup_hash(dup_key(cands, act, r, bc_of[r])) & mask); }
};

// table (may be null: no census): table_cap slots of which *n_table come back, as the launches left them; home[n_reads]: each read's home slot
template <class RT> int selftest_post_run(RT &rt, const IndexView &ix, int32_t n_reads, const int64_t *cand_off, const int64_t *cands, int64_t n_regs, const int64_t *regs,
                                          const int64_t *alns, const uint32_t *cigars, int64_t n_cig, const uint8_t *bases, const int32_t *lens, int32_t n_barcodes,
                                          const int64_t *bc_pair_off, int32_t penalty, const int64_t *cen_start, const int64_t *cen_end, void *post, void *split,
                                          int32_t *mm_ref, int32_t *mm_read, int64_t mm_cap, int64_t *n_mm, int32_t *table, int64_t table_cap, int32_t *n_table, int32_t *home)
{
	if (!bases || !post || !split || !mm_ref || !mm_read || !n_mm || mm_cap < 0 || (n_cig > 0 && !cigars) || (!cen_start) != (!cen_end)) return ARX_E_ARG;
	if (table && (!n_table || !home || table_cap < 0)) return ARX_E_ARG;
	if (!selftest_post_args_ok(ix, n_reads, cand_off, cands, n_regs, regs, alns, n_cig, lens, n_barcodes, bc_pair_off)) return ARX_E_ARG;
	for (int64_t g = 0; g < n_regs; ++g)
		for (int64_t j = 0; j < alns[g * SELFTEST_POST_ALN_W + 7]; ++j)
			if ((cigars[alns[g * SELFTEST_POST_ALN_W + 8] + j] >> 4) > (uint32_t)SELFTEST_POST_MAX_OPLEN) return ARX_E_ARG;
	const int R = n_reads;
	const int64_t NC = cand_off[R];
	if (table && table_cap < (int64_t)selftest_post_table_cap(R)) return ARX_E_TOO_LARGE;
	std::vector<int32_t> h_off((size_t)R + 1), h_bro((size_t)n_barcodes + 1);
	std::vector<Cand> h_cands((size_t)NC + 1);
	std::vector<Reg> h_regs((size_t)n_regs + 1, Reg());
	std::vector<Aln> h_alns((size_t)n_regs + 1, Aln());
	for (int r = 0; r <= R; ++r) h_off[r] = (int32_t)cand_off[r];
	for (int b = 0; b <= n_barcodes; ++b) h_bro[b] = (int32_t)(2 * bc_pair_off[b]);
	for (int64_t i = 0; i < NC; ++i) {
		const int64_t *c = cands + i * SELFTEST_POST_CAND_W;
		Cand x = Cand();
		x.reg = (int32_t)c[0]; x.read = (int32_t)c[1]; x.pos = c[2]; x.aend = c[3]; x.reversed = (int32_t)c[4]; x.rid = (int32_t)c[5]; x.score = (int32_t)c[6];
		x.mismatches = (int32_t)c[7]; x.indels = (int32_t)c[8]; x.soft_clipped = (int32_t)c[9]; x.soft_clipped_length = (int32_t)c[10]; x.lap2 = (int32_t)c[11];
		x.active = (int32_t)c[12]; x.is_proper = (int32_t)c[13]; x.mapq = (int32_t)c[14]; x.mol = (int32_t)c[15]; x.active_molecule = (int32_t)c[16];
		x.in_filtered = (int32_t)c[17]; memcpy(&x.sum_move, &c[18], 8); x.best_in_mol = (int32_t)c[19];
		h_cands[(size_t)i] = x;
	}
	for (int64_t g = 0; g < n_regs; ++g) {
		const int64_t *rg = regs + g * SELFTEST_POST_REG_W, *al = alns + g * SELFTEST_POST_ALN_W;
		h_regs[(size_t)g].qb = (int32_t)rg[2]; h_regs[(size_t)g].qe = (int32_t)rg[3];
		h_alns[(size_t)g].NM = (int32_t)al[6]; h_alns[(size_t)g].n_cigar = (int32_t)al[7]; h_alns[(size_t)g].cigar_off = (int32_t)al[8];
	}
	Pipeline<RT> pipe(rt, ix);
	typename Pipeline<RT>::DeviceBatch db = pipe.upload(bases, lens, R);
	typename Pipeline<RT>::Work w;
	int rc = ARX_OK;
	try {
		const int n_seqs = ix.n_seqs;
		RfaResult rfa;
		PostResult res;
		w.c_regs = rt.template alloc<Reg>((size_t)n_regs + 1); w.c_alns = rt.template alloc<Aln>((size_t)n_regs + 1); w.c_cig = rt.template alloc<uint32_t>((size_t)n_cig + 1);
		rfa.d_cands = rt.template alloc<Cand>((size_t)NC + 1); rfa.d_cand_off = rt.template alloc<int32_t>((size_t)R + 2); rfa.d_bc_read_off = rt.template alloc<int32_t>((size_t)n_barcodes + 1);
		rt.h2d(w.c_regs, h_regs.data(), sizeof(Reg) * (size_t)n_regs); rt.h2d(w.c_alns, h_alns.data(), sizeof(Aln) * (size_t)n_regs); rt.h2d(w.c_cig, cigars, 4 * (size_t)n_cig);
		rt.h2d(rfa.d_cands, h_cands.data(), sizeof(Cand) * (size_t)NC); rt.h2d(rfa.d_cand_off, h_off.data(), 4 * ((size_t)R + 1));
		rt.h2d(rfa.d_bc_read_off, h_bro.data(), 4 * ((size_t)n_barcodes + 1));
		if (cen_start) {
			rfa.d_cen_start = rt.template alloc<int64_t>((size_t)n_seqs + 1); rfa.d_cen_end = rt.template alloc<int64_t>((size_t)n_seqs + 1);
			rt.h2d(rfa.d_cen_start, cen_start, 8 * (size_t)n_seqs); rt.h2d(rfa.d_cen_end, cen_end, 8 * (size_t)n_seqs);
		}
		rfa.n_cands = NC; rfa.n_barcodes = n_barcodes; rfa.penalty = penalty;
		PostStage<RT>::run(pipe, db, w, rfa, res);
		rt.sync();
		*n_mm = res.n_mm;
		if (res.n_mm > mm_cap) rc = ARX_E_TOO_LARGE;
		else {
			static_assert(sizeof(CandPost) == 24 && sizeof(SplitRec) == 32, "the records arx_selftest_post hands out");
			PostStage<RT>::fetch(pipe, db, rfa, res, (CandPost *)post, (SplitRec *)split, mm_ref, mm_read);
			if (table) {
				if ((int64_t)res.cap > table_cap) rc = ARX_E_DEVICE; // (not the table this entry sized for)
				else {
					int32_t *d_home = rt.template alloc<int32_t>((size_t)R + 1);
					KSelftestPostHome kh{rfa.d_cands, res.d_act, res.d_bc_of, res.cap - 1, d_home};
					rt.launch_wide("selftest_post_home", R, kh);
					rt.sync();
					rt.d2h(table, res.d_table, 4 * (size_t)res.cap);
					rt.d2h(home, d_home, 4 * (size_t)R);
					*n_table = (int32_t)res.cap;
				}
			}
		}
	} catch (...) { pipe.release(db); throw; }
	pipe.release(db);
	return rc;
}

} // namespace arx

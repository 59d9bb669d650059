// selftest_reg2aln.h -- arx_selftest_reg2aln (include/arachne_amd.h) for any runtime: stage 6, Pipeline<RT>::stage_reg2aln itself (its slot loop, its
// kernels, compact()), on regions the caller made up.  The region rows are the restatement's (oracle/arx_oracle.h: ORA_REG_W; ora_reg2aln takes
// the same row).  What is filled of the batch and the work record is exactly what the stage and its kernels read: bases, base_off, lens, n_reads,
// max_len; P, preg_off, n_regs, pregs, err.  Included by arx_selftest.hip (HipRT) and by the host test double (tests/hostsim/sim.cpp).
#pragma once
#include <vector>
#include "../../include/arachne_amd.h"
#include "pipeline.h"

namespace arx {

constexpr int SELFTEST_R2A_REG_W = 20;          // oracle/arx_oracle.h: ORA_REG_W
constexpr int SELFTEST_R2A_MAX_RLEN = 4096;     // re - rb the entry accepts (the one-thread path refuses what its matrix cannot hold: ERR_POOL_OVERFLOW)
constexpr int SELFTEST_R2A_MAX_SLOTS = 1 << 20; // region slots: slot index x 1024 CIGAR words stays inside Aln::cigar_off
constexpr int SELFTEST_R2A_MAX_VAL = 1 << 24;   // |truesc|, w and the copied score fields: the band arithmetic stays far from 32 bits

// everything a kernel would index with, and everything bwa_gen_cigar2 rejects (bwa.c:126-134: the reference then reads a score it never set)
inline bool selftest_reg2aln_args_ok(const IndexView &ix, const int32_t *lens, int32_t n_reads, const int32_t *cap, const int32_t *n_regs, const int64_t *regs, int64_t *P_out)
{
	if (n_reads < 1 || !lens || !cap || !n_regs || ix.l_pac <= 0) return false;
	int64_t P = 0, tot = 0;
	for (int r = 0; r < n_reads; ++r) {
		if (lens[r] < 0 || lens[r] > MAX_READ_LEN || cap[r] < 0 || n_regs[r] < 0 || n_regs[r] > cap[r]) return false;
		for (int j = 0; j < n_regs[r]; ++j) {
			const int64_t *g = regs + (P + j) * SELFTEST_R2A_REG_W;
			const int64_t rb = g[0], re = g[1], qb = g[2], qe = g[3], L = ix.l_pac;
			if (!(0 <= qb && qb < qe && qe <= lens[r])) return false;
			if (!(0 <= rb && rb < re && re <= 2 * L) || (rb < L && re > L) || re - rb > SELFTEST_R2A_MAX_RLEN) return false;
			if (g[11] < 0 || g[11] > SELFTEST_R2A_MAX_VAL || g[6] < -SELFTEST_R2A_MAX_VAL || g[6] > SELFTEST_R2A_MAX_VAL) return false;
			for (int c = 4; c < 18; ++c) if (g[c] < -SELFTEST_R2A_MAX_VAL || g[c] > SELFTEST_R2A_MAX_VAL) return false;
		}
		P += cap[r]; tot += lens[r];
		if (P > SELFTEST_R2A_MAX_SLOTS) return false;
	}
	if (tot >= ((int64_t)1 << 31) - 64 || (P > 0 && !regs)) return false;
	*P_out = P;
	return true;
}

// census (may be null; census_cap int64 values): [0] final cig_w  [1] passes of the slot loop  [2] regions queued for the 16-lane kernel in the last
// pass  [3] regions too long for it  [4..8] queued per band class  [9] regions the class kernels handed on (-1: not kept)  [10] rows that follow
// [11] bit i set: value [i] is known to this runtime  then per queued region from [12] on: index among the compacted regions, band class, nw_need
constexpr int SELFTEST_R2A_CENSUS_HEAD = 12;

template <class RT> int selftest_reg2aln_run(RT &rt, const IndexView &ix, const uint8_t *bases, const int32_t *lens, int32_t n_reads, const int32_t *cap, const int32_t *n_regs,
                                             const int64_t *regs, int32_t *reg_off, void *alns, int64_t aln_cap, uint32_t *cigars, int64_t cig_cap, int64_t *n_cig,
                                             uint32_t *err, int64_t *census, int64_t census_cap)
{
	int64_t P = 0;
	if (!bases || !reg_off || !alns || !cigars || !n_cig || !err || aln_cap < 0 || cig_cap < 0 || (census && census_cap < SELFTEST_R2A_CENSUS_HEAD)) return ARX_E_ARG;
	if (!selftest_reg2aln_args_ok(ix, lens, n_reads, cap, n_regs, regs, &P)) return ARX_E_ARG;
	const int R = n_reads;
	std::vector<int32_t> h_off((size_t)R + 1), h_coff((size_t)R + 1);
	h_off[0] = h_coff[0] = 0;
	for (int r = 0; r < R; ++r) { h_off[r + 1] = h_off[r] + cap[r]; h_coff[r + 1] = h_coff[r] + n_regs[r]; }
	if (h_coff[R] > aln_cap) return ARX_E_TOO_LARGE;
	*n_cig = 0; *err = 0;
	if (P == 0) { for (int r = 0; r <= R; ++r) reg_off[r] = 0; if (census) for (int i = 0; i < SELFTEST_R2A_CENSUS_HEAD; ++i) census[i] = 0; return ARX_OK; }
	std::vector<Reg> h_regs((size_t)P + 1, Reg()); // (an unused slot holds zeros: the stage must not read it)
	for (int r = 0; r < R; ++r)
		for (int j = 0; j < n_regs[r]; ++j) {
			const int64_t *g = regs + ((int64_t)h_off[r] + j) * SELFTEST_R2A_REG_W;
			Reg x = Reg();
			x.rb = g[0]; x.re = g[1]; x.qb = (int32_t)g[2]; x.qe = (int32_t)g[3]; x.rid = (int32_t)g[4]; x.score = (int32_t)g[5]; x.truesc = (int32_t)g[6];
			x.sub = (int32_t)g[7]; x.alt_sc = (int32_t)g[8]; x.csub = (int32_t)g[9]; x.sub_n = (int32_t)g[10]; x.w = (int32_t)g[11]; x.seedcov = (int32_t)g[12];
			x.secondary = (int32_t)g[13]; x.secondary_all = (int32_t)g[14]; x.seedlen0 = (int32_t)g[15]; x.n_comp = (int32_t)g[16]; x.is_alt = (int32_t)g[17];
			h_regs[(size_t)h_off[r] + j] = x;
		}
	Pipeline<RT> pipe(rt, ix);
	Reg2AlnCensus cen;
	if (census) pipe.reg2aln_census = &cen;
	typename Pipeline<RT>::DeviceBatch db = pipe.upload(bases, lens, R);
	typename Pipeline<RT>::Work w;
	int rc = ARX_OK;
	try {
		w.err = rt.template alloc<uint32_t>(4); rt.memset0(w.err, 16);
		w.preg_off = rt.template alloc<int32_t>((size_t)R + 2); w.n_regs = rt.template alloc<int32_t>((size_t)R + 1);
		w.pregs = rt.template alloc<Reg>((size_t)P + 1);
		w.P = P;
		rt.h2d(w.preg_off, h_off.data(), 4 * ((size_t)R + 1)); rt.h2d(w.n_regs, n_regs, 4 * (size_t)R);
		rt.h2d(w.pregs, h_regs.data(), sizeof(Reg) * (size_t)P);
		const uint32_t e = (uint32_t)pipe.stage_reg2aln(db, w);
		rt.sync();
		*err = e;
		if (e & ERR_CIGAR_OVERFLOW) { // a CIGAR that 1024 words do not hold: the stage has returned without its dense results
			for (int r = 0; r <= R; ++r) reg_off[r] = 0;
		} else if (w.c_n_regs != h_coff[R]) rc = ARX_E_DEVICE;
		else if (w.c_n_cig > cig_cap) rc = ARX_E_TOO_LARGE;
		else {
			static_assert(sizeof(Aln) == 48, "the records arx_selftest_reg2aln hands out");
			rt.d2h(reg_off, w.c_reg_off, 4 * ((size_t)R + 1));
			rt.d2h(alns, w.c_alns, sizeof(Aln) * (size_t)w.c_n_regs);
			rt.d2h(cigars, w.c_cig, 4 * (size_t)w.c_n_cig);
			*n_cig = w.c_n_cig;
		}
	} catch (...) { pipe.release(db); throw; }
	pipe.release(db);
	if (rc != ARX_OK || !census) return rc;
	const int64_t nq = (int64_t)cen.list.size();
	if (census_cap < SELFTEST_R2A_CENSUS_HEAD + 3 * nq) return ARX_E_TOO_LARGE;
	census[0] = cen.cig_w; census[1] = cen.passes;
	for (int q = 0; q < 2 + NW_CLASSES; ++q) census[2 + q] = cen.count[q];
	census[9] = cen.punts; census[10] = nq;
	census[11] = 0x7ff & ~(cen.punts < 0 ? 1 << 9 : 0);
	for (int64_t k = 0; k < nq; ++k) {
		const int g = cen.list[(size_t)k];
		int lo = 0, hi = R;
		while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (h_off[mid] <= g) lo = mid; else hi = mid; }
		int64_t *o = census + SELFTEST_R2A_CENSUS_HEAD + 3 * k;
		o[0] = h_coff[lo] + (g - h_off[lo]); o[1] = cen.klass[(size_t)k]; o[2] = cen.need[(size_t)k];
	}
	return ARX_OK;
}

} // namespace arx

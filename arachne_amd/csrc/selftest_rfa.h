// selftest_rfa.h -- arx_selftest_rfa (include/arachne_amd.h) for any runtime: the placement stage, RfaStage<RT>::run itself, on alignments the
// caller made up.  The rows are the restatement's (oracle/arx_oracle_rfa.c: ora_rfa takes the same arrays); what is filled of the batch, the
// work record and the IndexView is exactly what RfaStage::run and its kernels read: n_reads and lens; n_regs, preg_off, c_reg_off, pregs
// (rb, re, rid, score), alns (rid, is_rev, NM, n_cigar), cig at cig_w words per region, counter; ann_off, l_pac, n_seqs.  Included by
// arx_selftest.hip (HipRT) and by the host test double (tests/hostsim/sim.cpp), which compile the same pipeline_rfa.h.
#pragma once
#include <optional>
#include <vector>
#include "../../include/arachne_amd.h"
#include "pipeline_rfa.h"

namespace arx {

constexpr int SELFTEST_REG_W = 20, SELFTEST_ALN_W = 12; // the restatement's int64 rows (oracle/arx_oracle.h: ORA_REG_W, ORA_ALN_W)

// everything a kernel would index with: checked on the host before anything is uploaded
inline bool selftest_rfa_args_ok(int32_t n_reads, const int64_t *reg_off, const int64_t *regs, const int64_t *alns, int64_t n_cig, const int32_t *lens, int32_t n_barcodes,
                                 const int64_t *bc_pair_off, int64_t l_pac, int32_t n_seqs, int64_t cand_cap, int *cig_w)
{
	if (n_reads <= 0 || (n_reads & 1) || n_barcodes <= 0 || n_seqs <= 0 || l_pac <= 0 || n_cig < 0) return false;
	if (!reg_off || !lens || !bc_pair_off || reg_off[0] != 0) return false;
	int64_t nc = 0;
	for (int r = 0; r < n_reads; ++r) {
		const int64_t n = reg_off[r + 1] - reg_off[r];
		if (n < 0 || lens[r] < 0 || lens[r] > MAX_READ_LEN) return false;
		nc += n ? n : 1;
	}
	const int64_t G = reg_off[n_reads];
	if (nc != cand_cap || nc >= ((int64_t)1 << 30) || (G > 0 && (!regs || !alns))) return false;
	int w = 1;
	for (int64_t g = 0; g < G; ++g) {
		const int64_t *rg = regs + g * SELFTEST_REG_W, *al = alns + g * SELFTEST_ALN_W;
		if (rg[4] < 0 || rg[4] >= n_seqs || al[1] < 0 || al[1] >= n_seqs) return false;
		if (rg[0] < 0 || rg[1] < 0 || rg[0] >= 2 * l_pac || rg[1] >= 2 * l_pac) return false;
		if (al[7] < 0 || al[7] > 64 || al[8] < 0 || al[8] + al[7] > n_cig) return false;
		if ((int)al[7] > w) w = (int)al[7];
	}
	if (bc_pair_off[0] != 0 || 2 * bc_pair_off[n_barcodes] != n_reads) return false;
	for (int b = 0; b < n_barcodes; ++b) if (bc_pair_off[b + 1] <= bc_pair_off[b]) return false;
	*cig_w = w;
	return true;
}

template <class RT> int selftest_rfa_run(RT &rt, int32_t n_reads, const int64_t *reg_off, const int64_t *regs, const int64_t *alns, const uint32_t *cigars, int64_t n_cig,
                                         const int32_t *lens, int32_t n_barcodes, const int64_t *bc_pair_off, const uint8_t *do_rfa, int32_t penalty, int64_t l_pac,
                                         const int64_t *ann_off, int32_t n_seqs, const int64_t *cen_start, const int64_t *cen_end, int32_t rfa_small, double mapq_guard,
                                         int32_t *cand_off, void *cands, int64_t cand_cap, void *bc_out, uint8_t *cls, int64_t *n_host_mapq)
{
	int cig_w = 1;
	if (!do_rfa || !ann_off || !cand_off || !cands || !bc_out || !cls || !n_host_mapq || (n_cig > 0 && !cigars) || (!cen_start) != (!cen_end)) return ARX_E_ARG;
	if (!selftest_rfa_args_ok(n_reads, reg_off, regs, alns, n_cig, lens, n_barcodes, bc_pair_off, l_pac, n_seqs, cand_cap, &cig_w)) return ARX_E_ARG;
	const int R = n_reads;
	const int64_t G = reg_off[R];
	std::vector<int32_t> h_off(R + 1), h_n(R);
	std::vector<Reg> h_regs((size_t)G + 1);
	std::vector<Aln> h_alns((size_t)G + 1);
	std::vector<uint32_t> h_cig(((size_t)G + 1) * cig_w, 0);
	for (int r = 0; r <= R; ++r) h_off[r] = (int32_t)reg_off[r];
	for (int r = 0; r < R; ++r) h_n[r] = h_off[r + 1] - h_off[r];
	for (int64_t g = 0; g < G; ++g) {
		const int64_t *rg = regs + g * SELFTEST_REG_W, *al = alns + g * SELFTEST_ALN_W;
		Reg x = Reg(); Aln a = Aln();
		x.rb = rg[0]; x.re = rg[1]; x.qb = (int32_t)rg[2]; x.qe = (int32_t)rg[3]; x.rid = (int32_t)rg[4]; x.score = (int32_t)rg[5]; x.truesc = (int32_t)rg[6];
		a.pos = al[0]; a.rid = (int32_t)al[1]; a.flag = (int32_t)al[2]; a.is_rev = (int32_t)al[3]; a.is_alt = (int32_t)al[4]; a.NM = (int32_t)al[6];
		a.n_cigar = (int32_t)al[7]; a.cigar_off = (int32_t)al[8]; a.score = (int32_t)al[9];
		h_regs[g] = x; h_alns[g] = a;
		for (int j = 0; j < a.n_cigar; ++j) h_cig[(size_t)g * cig_w + j] = cigars[al[8] + j];
	}
	IndexView ix = IndexView();
	int64_t *d_ann = rt.template alloc<int64_t>((size_t)n_seqs + 1);
	rt.h2d(d_ann, ann_off, 8 * (size_t)n_seqs);
	ix.ann_off = d_ann; ix.l_pac = l_pac; ix.n_seqs = n_seqs;
	PipelineSwitches sw;
	sw.rfa_small = rfa_small != 0;
	sw.mapq_guard = mapq_guard >= 0 ? std::optional<double>(mapq_guard) : std::nullopt;
	Pipeline<RT> pipe(rt, ix, sw);
	typename Pipeline<RT>::DeviceBatch db;
	typename Pipeline<RT>::Work w;
	int32_t *d_lens = rt.template alloc<int32_t>((size_t)R + 1), *d_off = rt.template alloc<int32_t>((size_t)R + 2), *d_n = rt.template alloc<int32_t>((size_t)R + 1);
	Reg *d_regs = rt.template alloc<Reg>((size_t)G + 1);
	Aln *d_alns = rt.template alloc<Aln>((size_t)G + 1);
	uint32_t *d_cig = rt.template alloc<uint32_t>(h_cig.size());
	rt.h2d(d_lens, lens, 4 * (size_t)R); rt.h2d(d_off, h_off.data(), 4 * (size_t)(R + 1)); rt.h2d(d_n, h_n.data(), 4 * (size_t)R);
	rt.h2d(d_regs, h_regs.data(), sizeof(Reg) * (size_t)G); rt.h2d(d_alns, h_alns.data(), sizeof(Aln) * (size_t)G); rt.h2d(d_cig, h_cig.data(), 4 * h_cig.size());
	db.n_reads = R; db.lens = d_lens;
	w.n_regs = d_n; w.preg_off = d_off; w.c_reg_off = d_off; w.pregs = d_regs; w.alns = d_alns; w.cig = d_cig; w.cig_w = cig_w;
	w.counter = rt.template alloc<int32_t>(4);
	RfaResult res;
	RfaStage<RT>::run(pipe, db, w, n_barcodes, bc_pair_off, do_rfa, penalty, cen_start, cen_end, lens, res);
	rt.sync();
	if (res.n_cands != cand_cap) return ARX_E_DEVICE;
	static_assert(sizeof(Cand) == 96 && sizeof(RfaBarcodeOut) == 16, "the records arx_selftest_rfa hands out");
	RfaStage<RT>::fetch(pipe, db, res, cand_off, (Cand *)cands);
	memcpy(bc_out, res.bc.data(), sizeof(RfaBarcodeOut) * (size_t)n_barcodes);
	memcpy(cls, res.cls.data(), (size_t)n_barcodes);
	*n_host_mapq = res.n_host_mapq;
	return ARX_OK;
}

} // namespace arx

// selftest_ext.h -- arx_selftest_ext_stage (include/arachne_amd.h) for any runtime: stage 4, Pipeline<RT>::stage_extend itself (KExtInit, the round
// loop over KExtStep and run_extend, KExtGather, KDedup), on chains and seeds the caller made up.  The chain and seed rows are the restatement's
// (oracle/arx_oracle.h: ora_chains hands them out, ora_chain2aln takes the same rows), the region rows too (ORA_REG_W).  What is filled of the batch and
// the work record is exactly what the stage and its kernels read: bases, base_off, lens, n_reads, max_len; T, occ_off, n_chain, cout, sout, err.
// Included by arx_selftest.hip (HipRT) and by the host test double (tests/hostsim/sim.cpp).
#pragma once
#include <vector>
#include "../../include/arachne_amd.h"
#include "pipeline.h"

namespace arx {

constexpr int SELFTEST_EXT_REG_W = 20;           // oracle/arx_oracle.h: ORA_REG_W
constexpr int SELFTEST_EXT_ROUND_W = 2 + EXT_CLASSES;
constexpr int64_t SELFTEST_EXT_MAX_SLOTS = 1 << 22; // chain and seed slots of one call

inline void selftest_ext_put_reg(int64_t *r, const Reg &p)
{
	uint32_t fb;
	memcpy(&fb, &p.frac_rep, 4);
	r[0] = p.rb; r[1] = p.re; r[2] = p.qb; r[3] = p.qe; r[4] = p.rid; r[5] = p.score; r[6] = p.truesc; r[7] = p.sub; r[8] = p.alt_sc; r[9] = p.csub; r[10] = p.sub_n;
	r[11] = p.w; r[12] = p.seedcov; r[13] = p.secondary; r[14] = p.secondary_all; r[15] = p.seedlen0; r[16] = p.n_comp; r[17] = p.is_alt; r[18] = fb; r[19] = 0;
}

// What mem_chain2aln accepts (the reference's assert(c->rid == rid) and its fetches): every seed of a chain in one contig and strand, rid that contig,
// 0 <= qbeg, qbeg + len <= l_query, len >= 1, score == len; a chain's seeds are rows [seed_off, seed_off + n) of its read's seed rows, chain after chain
inline bool selftest_ext_args_ok(int64_t l_pac, int32_t n_seqs, const int64_t *ann_off, const int32_t *ann_len, const uint8_t *bases, const int32_t *lens, int32_t n_reads,
                                 const int32_t *n_chain, const int64_t *chains, const int32_t *n_seed, const int64_t *seeds, int64_t *T_out)
{
	if (n_reads < 1 || !lens || !n_chain || !n_seed || !bases || l_pac <= 0) return false;
	int64_t c0 = 0, s0 = 0, T = 0, tot = 0;
	for (int r = 0; r < n_reads; ++r) {
		if (lens[r] < 1 || lens[r] > MAX_READ_LEN || n_chain[r] < 0 || n_seed[r] < 0) return false;
		for (int k = 0; k < lens[r]; ++k) if (bases[tot + k] > 4) return false;
		if ((n_chain[r] > 0 && !chains) || (n_seed[r] > 0 && !seeds)) return false;
		int64_t next = 0; // the chains' seed rows follow each other, as mem_chain's do: a chain's regions go to the slots of its own seeds
		for (int ci = 0; ci < n_chain[r]; ++ci) {
			const int64_t *c = chains + 8 * (c0 + ci);
			if (c[2] < 0 || c[3] < next || c[3] + c[2] > n_seed[r]) return false;
			next = c[3] + c[2];
			if (c[2] > 0 && (c[1] < 0 || c[1] >= n_seqs)) return false;
			bool rev0 = false;
			for (int64_t j = 0; j < c[2]; ++j) {
				const int64_t *s = seeds + 4 * (s0 + c[3] + j);
				const int64_t b = s[0], e = s[0] + s[2];
				const bool rev = b >= l_pac;
				if (s[2] < 1 || s[1] < 0 || s[1] + s[2] > lens[r] || s[3] != s[2]) return false;
				if (b < 0 || e > 2 * l_pac || (b < l_pac && e > l_pac)) return false;
				if (j == 0) rev0 = rev; else if (rev != rev0) return false;
				const int64_t fb = rev ? 2 * l_pac - e : b, fe = rev ? 2 * l_pac - b : e;
				if (fb < ann_off[c[1]] || fe > ann_off[c[1]] + ann_len[c[1]]) return false;
			}
		}
		c0 += n_chain[r]; s0 += n_seed[r]; tot += lens[r];
		T += n_chain[r] > n_seed[r] ? n_chain[r] : n_seed[r]; // a read's slice of the pools holds its chains (one slot each) and its seeds
		if (T > SELFTEST_EXT_MAX_SLOTS) return false;
	}
	if (tot >= ((int64_t)1 << 31) - 64) return false;
	*T_out = T;
	return true;
}

// ext_off / core_off: n_reads + 1 offsets into ext_regs / core_regs (rows of SELFTEST_EXT_REG_W; reg_cap rows each, the seeds' number suffices).
// stats: [0] n_ext_tasks  [1] ext_rounds  [2] rounds the census saw (rows of `rounds`: round, chains active after it, tasks per length class)  [3] chains.
// done_round, chain_n_regs: per chain, in the order of the chain rows
template <class RT> int selftest_ext_run(RT &rt, const IndexView &ix, const uint8_t *bases, const int32_t *lens, int32_t n_reads, const int32_t *n_chain, const int64_t *chains,
                                         const int32_t *n_seed, const int64_t *seeds, const uint32_t *frac_rep_bits, int32_t *ext_off, int64_t *ext_regs, int32_t *core_off,
                                         int64_t *core_regs, int64_t reg_cap, int32_t *core_clean, int64_t *stats, int32_t *rounds, int64_t rounds_cap, int32_t *done_round,
                                         int32_t *chain_n_regs, uint32_t *err)
{
	if (!ext_off || !ext_regs || !core_off || !core_regs || !core_clean || !stats || !rounds || !done_round || !chain_n_regs || !err || !frac_rep_bits || reg_cap < 0 || rounds_cap < 0)
		return ARX_E_ARG;
	if (ix.l_pac <= 0 || ix.n_seqs < 1) return ARX_E_ARG;
	std::vector<int64_t> ann_off((size_t)ix.n_seqs); std::vector<int32_t> ann_len((size_t)ix.n_seqs);
	rt.d2h(ann_off.data(), ix.ann_off, 8 * (size_t)ix.n_seqs); rt.d2h(ann_len.data(), ix.ann_len, 4 * (size_t)ix.n_seqs);
	int64_t T = 0;
	if (!selftest_ext_args_ok(ix.l_pac, ix.n_seqs, ann_off.data(), ann_len.data(), bases, lens, n_reads, n_chain, chains, n_seed, seeds, &T)) return ARX_E_ARG;
	const int R = n_reads;
	std::vector<int32_t> h_occ((size_t)R + 2, 0);
	std::vector<Chain> h_ch((size_t)T + 1, Chain()); // (an unused slot holds zeros: the stage must not read it)
	std::vector<Seed> h_sd((size_t)T + 1, Seed());
	int64_t c0 = 0, s0 = 0, n_seeds = 0;
	for (int r = 0; r < R; ++r) {
		const int g0 = h_occ[(size_t)r];
		for (int ci = 0; ci < n_chain[r]; ++ci) {
			const int64_t *c = chains + 8 * (c0 + ci);
			Chain x = Chain();
			x.pos = c[0]; x.rid = (int32_t)c[1]; x.n = (int32_t)c[2]; x.seed_off = g0 + (int32_t)c[3]; x.w = (int32_t)c[4]; x.kept = (int32_t)c[5]; x.first = (int32_t)c[6];
			x.is_alt = (int32_t)c[7]; x.head = x.tail = -1;
			memcpy(&x.frac_rep, &frac_rep_bits[r], 4);
			h_ch[(size_t)g0 + ci] = x;
		}
		for (int j = 0; j < n_seed[r]; ++j) {
			const int64_t *s = seeds + 4 * (s0 + j);
			Seed x; x.rbeg = s[0]; x.qbeg = (int32_t)s[1]; x.len = (int32_t)s[2];
			h_sd[(size_t)g0 + j] = x;
		}
		c0 += n_chain[r]; s0 += n_seed[r]; n_seeds += n_seed[r];
		h_occ[(size_t)r + 1] = g0 + (n_chain[r] > n_seed[r] ? n_chain[r] : n_seed[r]);
	}
	if (n_seeds > reg_cap) return ARX_E_TOO_LARGE;
	const int64_t NCH = c0;
	Pipeline<RT> pipe(rt, ix);
	ExtCensus cen;
	pipe.ext_census = &cen;
	typename Pipeline<RT>::DeviceBatch db = pipe.upload(bases, lens, R);
	typename Pipeline<RT>::Work w;
	BatchResult res;
	int rc = ARX_OK;
	try {
		w.err = rt.template alloc<uint32_t>(4); rt.memset0(w.err, 16);
		w.occ_off = rt.template alloc<int32_t>((size_t)R + 2); w.n_chain = rt.template alloc<int32_t>((size_t)R + 1);
		w.cout = rt.template alloc<Chain>((size_t)T + 1); w.sout = rt.template alloc<Seed>((size_t)T + 1);
		w.T = T;
		rt.h2d(w.occ_off, h_occ.data(), 4 * ((size_t)R + 1)); rt.h2d(w.n_chain, n_chain, 4 * (size_t)R);
		rt.h2d(w.cout, h_ch.data(), sizeof(Chain) * ((size_t)T + 1)); rt.h2d(w.sout, h_sd.data(), sizeof(Seed) * ((size_t)T + 1));
		pipe.stage_extend(db, w, res);
		rt.sync();
		*err = pipe.read_err(w);
		std::vector<int32_t> n_core((size_t)R);
		std::vector<Reg> core((size_t)T + 1);
		rt.d2h(n_core.data(), w.n_core, 4 * (size_t)R);
		rt.d2h(core_clean, w.core_clean, 4 * (size_t)R);
		rt.d2h(core.data(), w.regs, sizeof(Reg) * (size_t)T);
		if ((int64_t)cen.done_round.size() != NCH || (int64_t)cen.n_ext.size() != R) rc = ARX_E_DEVICE;
		else if ((int64_t)cen.rounds.size() > rounds_cap * SELFTEST_EXT_ROUND_W) rc = ARX_E_TOO_LARGE;
		else {
			ext_off[0] = core_off[0] = 0;
			for (int r = 0; r < R && rc == ARX_OK; ++r) {
				const int ne = cen.n_ext[(size_t)r], nc = n_core[(size_t)r], room = h_occ[(size_t)r + 1] - h_occ[(size_t)r];
				if (ne < 0 || ne > room || nc < 0 || nc > ne) { rc = ARX_E_DEVICE; break; }
				for (int i = 0; i < ne; ++i) selftest_ext_put_reg(ext_regs + (int64_t)SELFTEST_EXT_REG_W * (ext_off[r] + i), cen.regs[(size_t)h_occ[(size_t)r] + i]);
				for (int i = 0; i < nc; ++i) selftest_ext_put_reg(core_regs + (int64_t)SELFTEST_EXT_REG_W * (core_off[r] + i), core[(size_t)h_occ[(size_t)r] + i]);
				ext_off[r + 1] = ext_off[r] + ne; core_off[r + 1] = core_off[r] + nc;
			}
			for (size_t i = 0; i < cen.rounds.size(); ++i) rounds[i] = cen.rounds[i];
			for (int64_t g = 0; g < NCH; ++g) { done_round[g] = cen.done_round[(size_t)g]; chain_n_regs[g] = cen.n_regs[(size_t)g]; }
			stats[0] = res.n_ext_tasks; stats[1] = res.ext_rounds; stats[2] = (int64_t)(cen.rounds.size() / SELFTEST_EXT_ROUND_W); stats[3] = NCH;
		}
	} catch (...) { pipe.release(db); throw; }
	pipe.release(db);
	return rc;
}

} // namespace arx

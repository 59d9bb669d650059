/*
 * oracle/arx_oracle.h -- TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement (plain C, written from scratch) of the reference's per-pair hot path:
 * FM-index seeding, chaining, banded extension, mate rescue and CIGAR generation, exactly as
 * pdimens/arachne drives the vendored BWA 0.7.16a core through its cgo bridge
 * (/root/reference/src/gobwa/gobwa.go:226-337,400-415).  Every function cites the reference
 * file:line it follows.  The product (arachne_amd/, libarachne_amd.so) never includes, links or
 * calls anything in this directory; only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg do, and only as the checker.
 *
 * Parity pin: this restatement is checked bit-for-bit against oracle/_ref/libbwaref.so (the
 * reference's own C sources compiled in place) by tests/test_oracle_vs_ref.py, and against the
 * committed vectors in tests/golden/ (generated from that .so by tests/golden/make_golden.py).
 */
#ifndef ARX_ORACLE_H
#define ARX_ORACLE_H
#include <stdint.h>

#define ORA_REG_W 20 /* same row layout as oracle/ref_driver.c */
#define ORA_ALN_W 12

typedef struct ora_ctx ora_ctx_t;

/* instrumentation: algorithmic work counters accumulated over a batch */
typedef struct {
	int64_t n_reads;
	int64_t ext_same_block;  /* E1: bwt_extend calls whose k-1 and k-1+size share one Occ block */
	int64_t ext_two_block;   /* E2: ... fall in two blocks */
	int64_t sa_lookups;      /* N_sa */
	int64_t sa_lf_steps;     /* S: LF steps over all bwt_sa calls */
	int64_t n_regs;          /* regs produced (post rescue) */
	int64_t cells_extend;    /* ksw_extend2 cell updates */
	int64_t cells_u8;        /* ksw_u8 cell updates (qlen_padded x rows) */
	int64_t cells_global;    /* ksw_global2 cell updates */
	int64_t n_extend_calls, n_u8_calls, n_global_calls;
	int64_t ext3_same_block, ext3_two_block; /* the share of E1 / E2 spent in the third seeding pass (bwt_seed_strategy1) */
	int64_t extb_same_block, extb_two_block; /* the share spent in backward extensions (the backward sweeps of bwt_smem1a) */
	int64_t n_smem_calls;                    /* bwt_smem1a calls (first pass + re-seeding) */
	int64_t sa_lf_steps8;                    /* LF steps of the same lookups up to the first row that is a multiple of 8 */
	int64_t sa_lf_steps4;                    /* ... of 4 (the product's suffix-array sample since round 3) */
	int64_t ext_rows_qlen, ext_rows_cols;    /* ksw_extend2: rows computed x query length, and x the columns of the device kernel's length class (16 lanes x C) */
} ora_counters_t;

#ifdef __cplusplus
extern "C" {
#endif

ora_ctx_t *ora_open(const char *prefix);            /* reads <prefix>.{bwt,sa,pac,ann,amb,alt} */
void ora_close(ora_ctx_t *c);
int64_t ora_l_pac(ora_ctx_t *c);
int64_t ora_seq_len(ora_ctx_t *c);
int64_t ora_primary(ora_ctx_t *c);
int ora_n_seqs(ora_ctx_t *c);
void ora_counters(ora_ctx_t *c, ora_counters_t *out, int reset);

/* per-function known-answer entry points (same signatures as the ref_* ones in ref_driver.c) */
void ora_occ4(ora_ctx_t *c, int n, const uint64_t *k, uint64_t *out);
void ora_extend(ora_ctx_t *c, int n, const uint64_t *ik3, int is_back, uint64_t *ok12);
void ora_sa(ora_ctx_t *c, int n, const uint64_t *k, uint64_t *out);
int ora_collect_intv(ora_ctx_t *c, int len, const uint8_t *seq, uint64_t *out, int cap);
/* The shape of a read's seeding work, from the same run of mem_collect_intv that fills intv (the intervals ora_collect_intv returns): one row
 * of ORA_SHAPE_W numbers per bwt_smem1a call (passes 1 and 2) and per start of the third pass, in call order.  Tests assert from these rows
 * that their inputs reach the rare paths of the product's seeding kernels.  Columns:
 *  0 pass (1, 2, 3)   1 start x   2 min_intv   3 length of the forward list   4 depth (bases from x) at which the forward interval first holds
 *  one occurrence with a base left to try, -1: never   5 rows of the backward sweep that kept something   6 the widest of them   7 backward
 *  extensions   8 a row of ONE interval with ONE occurrence occurs (min_intv = 1)   9 the product's table jump at depth kf (passes 1, 2) or of
 *  the third pass (k3 != 0): 0 taken, 1 refused for an ambiguous base, 2 for the end of the read, 3 because the kf-mer occurs fewer than
 *  min_intv times, -1 no table   10 rows (as in 5) of more than 16 intervals   11 the call's return value (the next start).
 * kf and k3 only enter column 9.  Returns the number of rows (rows beyond cap_s are counted, not stored). */
#define ORA_SHAPE_W 12
int ora_seed_shapes(ora_ctx_t *c, int len, const uint8_t *seq, int kf, int k3, int64_t *shapes, int cap_s, uint64_t *intv, int cap_i, int *n_intv);
/* The shape of a pair's list work, from one run of the pair path (counts only; nothing the path computes depends on them).  Tests assert from
 * these that their inputs reach the lane, word and LDS-class edges of the product's wavefront-per-item list kernels.
 * reads: two rows of ORA_LSHAPE_W numbers, read 1 then read 2:
 *  0 seed occurrences mem_chain takes (its loop's iterations, at most max_occ per interval)   1 chains built   2 chains mem_chain_flt sorts
 *  3 chains it keeps (after the max_chain_extend cut)   4 the highest kept rank (index into kept_idx) of a chain that dropped another, -1: no
 *  drop   5, 6, 7 drops decided at kept rank 62, 63, 64   8 the longest run of equal weights among the sorted chains
 *  9 regions before mem_sort_dedup_patch   10 regions after it   11 entries its redundancy loop removes   12 those of them whose index is >= 64
 *  and whose stopper lies in another 64-entry word   13 identical (score, rb, qb) neighbours its final sort drops at an index that is a multiple
 *  of 64   14 mem_patch_reg calls that reach their alignment   15 those that merge   16 the most chains kept at the time of a drop
 *  17 drops   18 identical neighbours dropped   19 regions after rescue   20 of the entries in 11, those dropped as the LATER of a pair (the
 *  earlier one scores higher and stops the scan)   21 those of them whose stopper lies in another 64-entry word.
 * ins: one row of ORA_LINS_W numbers per region mem_matesw inserts, in call order:
 *  0 the list (0: read 1's)   1 its length before the insertion   2 the position the region is inserted at   3 an entry of the list ties with
 *  it (equal re, or equal score, rb and qb)   4 entries the pass that follows removes   5 index of the anchor in the mate's list   6 two
 *  entries that end before the region, are redundant with it and score higher share the greatest end and lie in different 64-entry steps.
 * Returns the number of insertions (rows beyond cap_ins are counted, not stored). */
#define ORA_LSHAPE_W 24
#define ORA_LINS_W 8
int ora_list_shapes(ora_ctx_t *c, int l1, const uint8_t *s1, int l2, const uint8_t *s2, int score_delta, int64_t *reads, int64_t *ins, int cap_ins);
int ora_chains(ora_ctx_t *c, int len, const uint8_t *seq, int do_flt, int64_t *chains, int cap_c, int64_t *seeds, int cap_s, int *n_seeds_out, uint32_t *frac_rep_bits);
void ora_ksw_extend2(ora_ctx_t *c, int qlen, const uint8_t *q, int tlen, const uint8_t *t, int w, int end_bonus, int zdrop, int h0, int *out);
void ora_ksw_align2(ora_ctx_t *c, int qlen, const uint8_t *q, int tlen, const uint8_t *t, int xtra, int *out);
int ora_ksw_global2(ora_ctx_t *c, int qlen, const uint8_t *q, int tlen, const uint8_t *t, int w, int *score, uint32_t *cigar, int cap);
int ora_align1(ora_ctx_t *c, int len, const uint8_t *seq, int64_t *regs, int cap);
int64_t ora_fetch_seq(ora_ctx_t *c, int64_t *beg, int64_t mid, int64_t *end, int *rid, uint8_t *out, int64_t cap);

/* mem_reg2aln (bwamem.c:1086-1156) on one region row and its read: the aln row (cigar_off 0), the CIGAR (returns n_cigar; words beyond cap are not
 * stored) and the shape of the work, from the same run.  The row must be one bwa_gen_cigar2 accepts (bwa.c:126-134); mem_reg2aln is a pure function
 * of (row, read, index), so any such row is legal input.  shape, ORA_R2A_W numbers:
 *  0 bwa_gen_cigar2 calls (1..3)   1-3 the band w_ each call was given, -1: no such call   4-6 the band ksw_global2 ran with (-1: the gap-free
 *  shortcut)   7-9 its n_col = min(l_query, 2w + 1) (0: the shortcut)   10-12 the call's score   13 n_cigar as bwa_gen_cigar2 left it (before the
 *  squeeze and the clips)   14 a deletion was squeezed: 1 the leading one, 2 the trailing one   15, 16 clip5, clip3   17 why the loop stopped,
 *  as bits: 1 score == last_sc, 2 the band had reached opt->w << 2 (both can hold); 0: its own condition (three calls, or a score within opt->a of truesc).
 *  18 the largest n_cigar any of the calls left (a narrow band's detour can take more operations than the final CIGAR). */
#define ORA_R2A_W 19
int ora_reg2aln(ora_ctx_t *c, int l_query, const uint8_t *query, const int64_t *reg_row, int64_t *aln_row, uint32_t *cigar, int cap, int64_t *shape);

/* mem_chain2aln (bwamem.c:632-786) over every chain of one read, in order, on chains the caller wrote: chain rows (8 int64) and seed rows (4 int64)
 * as ora_chains hands them out, frac_rep as its bits.  mem_chain2aln is a pure function of its rows, the read and the index, so the seeds need not be
 * what seeding would find.  Legal input is what the reference's assert(c->rid == rid) and its fetches accept: every seed of a chain in one contig and
 * strand, rid that contig, 0 <= qbeg, qbeg + len <= l_query, len >= 1 (and score == len, as mem_chain sets it); anything else returns -1.
 * regs: the regions after the last chain, BEFORE mem_sort_dedup_patch (returns their number; rows beyond cap_r are not stored).
 * calls: one row of ORA_C2A_CALL_W numbers per ksw_extend2 call, in call order (*n_calls; rows beyond cap_calls are counted, not stored):
 *  0 chain   1 seed (index within the chain)   2 side (0 left, 1 right)   3 qlen   4 tlen   5 w   6 h0   7 score   8 qle   9 tle   10 gtle   11 gscore   12 max_off.
 * shapes (may be null): one row of ORA_C2A_SHAPE_W numbers per chain, from the same run:
 *  0 regions appended   1 seeds skipped   2 seeds an earlier region explains but an overlapping off-diagonal seed keeps (bwamem.c:690-706)
 *  3, 4 left, right DPs   5, 6 second-band tries, left, right   7, 8 to-end branches (gscore taken), left, right   9 calls with tlen == 0
 *  10 calls with 0 < tlen < qlen   11, 12 the window [rmax0, rmax1)   13 what moved it, as bits: 1 the clamp at zero, 2 at l_pac, 4 at 2 * l_pac,
 *  8 the contig's boundary   14 earlier non-empty chains whose window holds one of this chain's seeds   15 the last of them (-1: none). */
#define ORA_C2A_CALL_W 13
#define ORA_C2A_SHAPE_W 16
int ora_chain2aln(ora_ctx_t *c, int l_query, const uint8_t *query, int n_chains, const int64_t *chains, int n_seeds, const int64_t *seeds, uint32_t frac_rep_bits,
                  int64_t *regs, int cap_r, int64_t *calls, int cap_calls, int *n_calls, int64_t *shapes);
/* mem_sort_dedup_patch (bwamem.c:437-489) and the is_alt marks of mem_align1_core on region rows, in place; returns the number left */
int ora_sort_dedup_patch(ora_ctx_t *c, int l_query, const uint8_t *query, int n, int64_t *regs);

/* the per-pair path */
double ora_batch_run(ora_ctx_t *c, int64_t n_pairs, const uint8_t *seqs, const int32_t *lens, int score_delta, int n_threads);
void ora_batch_get(ora_ctx_t *c, int64_t *n_reads, int64_t *n_regs, int64_t *n_cig, int64_t **reg_off, int64_t **regs, int64_t **alns, uint32_t **cigars);

/* the Go half (arx_oracle_rfa.c): candidate post-processing, RFA placement, MAPQ.  Row layout ORA_CAND_W = 20 int64:
 * reg read pos aend reversed rid score mismatches indels soft_clipped soft_clipped_length lap2 active is_proper mapq
 * molecule_id active_molecule in_filtered sum_move (the double's bits) best_in_mol (after scrapMolecules) */
#define ORA_CAND_W 20
int64_t ora_rfa(int64_t n_reads, const int64_t *reg_off, const int64_t *regs, const int64_t *alns, const uint32_t *cigars, const int32_t *lens,
                int n_barcodes, const int64_t *bc_pair_off, const uint8_t *do_rfa, int penalty, int64_t l_pac, const int64_t *ann_off,
                const int64_t *cen_start, const int64_t *cen_end, int64_t *cand_rows, int64_t *cand_off);

/* passes between placement and the BAM records (CIGAR walk, markDuplicates, CheckSplitReads); rows documented at the function */
#define ORA_POST_W 6
#define ORA_SPLIT_W 7
int64_t ora_post(ora_ctx_t *ctx, int64_t n_reads, const int64_t *regs, const int64_t *alns, const uint32_t *cigars, const uint8_t *bases, const int32_t *lens,
                 int n_barcodes, const int64_t *bc_pair_off, int penalty, const int64_t *ann_off, const int64_t *cen_start, const int64_t *cen_end,
                 const int64_t *cand_rows, const int64_t *cand_off, int64_t *post_rows, int64_t *split_rows, int32_t *mm_ref, int32_t *mm_read, int64_t mm_cap);

#ifdef __cplusplus
}
#endif
#endif

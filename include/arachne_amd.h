/*
 * arachne_amd.h -- C ABI of libarachne_amd.so, the MI355X (gfx950) implementation of Arachne's per-barcode
 * alignment hot path.  Plain pointers and sizes only; no torch / HIP types cross this boundary.
 *
 * What it replaces in the reference (pdimens/arachne @ 2025-09-05), whose Go code reaches the BWA C core one
 * read / one candidate at a time through cgo (src/gobwa/gobwa.go:7-13, src/gobwa/bwa_bridge.h:35-39):
 *
 *   arx_open           <- bwa_idx_load(path, BWA_IDX_ALL) + mem_opt_init()      gobwa.go:128-152 (GoBwaLoadReference, GoBwaAllocSettings)
 *   arx_contigs        <- direct field reads of bwaidx_t.bns / bntann1_t        gobwa.go:28-39,420-432 (GetReferenceContigsInfo, EnumerateContigs)
 *   arx_batch_create   <- SequenceConvert (nst_nt4_table) per read              gobwa.go:159-167; the caller passes 0..4 codes
 *   arx_batch_run      <- per pair: mem_align1_core x2, the two mem_matesw loops, InterpretAlign           gobwa.go:226-337 (GoBwaMemMateSW)
 *                         per candidate: mem_reg2aln                                                      gobwa.go:400-415 (GoBwaSmithWaterman)
 *                         i.e. loops A and B of DoRFAForOneBarcode               src/aligner/aligner.go:1633-1715,1484-1501
 *   arx_batch_fetch    <- mem_alnreg_v / mem_aln_t returned by value + Arena     gobwa.go:107-126,191,326-327,411-412
 *   arx_batch_free     <- Arena.Free                                             aligner.go:475,500
 *
 * Errors: every entry returns ARX_OK (0) or a negative code and never aborts the process (the reference asserts /
 * err_fatals); arx_last_error() gives the text.  A context may be shared by threads that each own their batches.
 * Results are bit-identical to the reference C core: same regions in the same order, same CIGAR/NM/pos/strand.
 */
#ifndef ARACHNE_AMD_H
#define ARACHNE_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct arx_ctx arx_ctx;
typedef struct arx_batch arx_batch;

enum { ARX_OK = 0, ARX_E_OPEN = -1, ARX_E_ARG = -2, ARX_E_DEVICE = -3, ARX_E_TOO_LARGE = -4, ARX_E_IO = -5 };

/* last_stage values for arx_batch_run: stop after a stage to inspect intermediate results */
enum { ARX_STAGE_SEED = 1, ARX_STAGE_CHAIN = 2, ARX_STAGE_EXTEND = 3, ARX_STAGE_RESCUE = 4, ARX_STAGE_ALN = 5 };

/* mem_alnreg_t (bwa/bwamem.h:66-87) without `hash` (always 0 on this path); frac_rep keeps its float bits */
typedef struct {
	int64_t rb, re;                 /* [rb,re) on the forward+reverse reference */
	int32_t qb, qe, rid, score, truesc, sub, alt_sc, csub, sub_n, w, seedcov, secondary, secondary_all, seedlen0, n_comp, is_alt;
	float frac_rep;
	int32_t pad;
} arx_reg;

/* mem_aln_t (bwa/bwamem.h:97-108) without XA and mapq (never read by Arachne) */
typedef struct {
	int64_t pos;                    /* 0-based leftmost position on contig rid */
	int32_t rid, flag, is_rev, is_alt, NM, n_cigar, cigar_off /* into the cigar array of the batch */, score, sub, alt_sc;
} arx_aln;

typedef struct { int64_t pos; int32_t rid, n, seed_off, w, kept, first, is_alt, head, tail; float frac_rep; } arx_chain; /* mem_chain_t */
typedef struct { int64_t rbeg; int32_t qbeg, len; } arx_seed;                                                         /* mem_seed_t  */

/* Builds <prefix>.{bwt,sa,pac,ann,amb} from a plain-text FASTA, byte-identical to the reference's `bwa index`
 * (bwa/bwtindex.c:251-316 bwa_idx_build).  FASTA parsing and the .pac / .ann / .amb files are host work; BWT and suffix array are sorted
 * in HBM when a HIP device is visible (any genome size the HBM holds: GRCh38 in ~10 s) and by a 32-bit host sorter otherwise (2 * l_pac < 2^31;
 * ARX_INDEX_HOST=1 forces it, ARX_INDEX_DEVICE=k picks the device) -- same bytes either way.  msg (may be NULL) receives the error text. */
int arx_index_build(const char *fasta, const char *prefix, char *msg, int32_t msg_cap);
/* Where the calling thread's last arx_index_build spent its time, in seconds: secs[0] the FASTA loop (parse and pack), secs[1] writing .pac,
 * .ann and .amb, secs[2] the suffix sort with .bwt and .sa.  Timing only; a call that failed leaves what it reached. */
int arx_index_build_times(double *secs);

/* The same five files, the FASTA read and packed on the GPU (replaces the host loop of bns_fasta2bntseq, bntseq.c:227-328; dev_fapack.h,
 * hip_fapack.h).  The FASTA may be plain text, ordinary gzip (both through zlib on a reader thread) or BGZF (read as it is and inflated on the
 * device), as the reference's gzopen takes them.  The packed forward strand, the contig table and the hole table are made on `device` window by
 * window and the suffix sorter takes the strand where it lies.  The bytes are arx_index_build's for the plain-text form of the same FASTA.
 *   flags   ARX_INDEX_PACK_ONLY: .pac, .ann and .amb only.  Unknown bits: ARX_E_ARG.
 *   stats   (may be NULL) ARX_INDEX_N_STATS values: [0] l_pac  [1] contigs  [2] holes  [3] ambiguous bases  [4] text bytes  [5] compressed bytes
 *           read (the file's size)  [6] windows; microseconds: [7] waiting for the reader  [8] upload + inflate  [9] pack  [10] .pac fetch + write
 *           [11] .ann / .amb  [12] suffix sort + .bwt / .sa  [13] total.
 * Every file is written as <file>.tmp and renamed when all are complete; a failing call leaves nothing.  There is no CPU fallback: no such
 * device is ARX_E_DEVICE with a text.  ARX_E_ARG: null paths, unknown flags; ARX_E_IO: the FASTA cannot be read, a BGZF block does not
 * inflate, zlib reports an error (a truncated gzip stream), a file cannot be written; ARX_E_OPEN, with arx_index_build's texts: a base
 * before the first '>', no base at all; ARX_E_TOO_LARGE: a contig of more than 2^31 - 1 bases, more than 2^31 - 1 contigs or holes (the host
 * loop overflows silently there), or buffers the device does not hold.  msg (may be NULL) receives the text. */
enum { ARX_INDEX_PACK_ONLY = 1 };
enum { ARX_INDEX_N_STATS = 14 };
int arx_index_build_ex(int32_t device, const char *fasta, const char *prefix, int32_t flags, int64_t *stats, char *msg, int32_t msg_cap);

/* The pack of arx_index_build_ex on a text in host memory, in windows of window_bytes (0: the default, 2^24; otherwise at least 64 and at
 * most 2^24, ARX_E_ARG outside).  pac[pac_cap] receives the packed bases, (l_pac + 3) / 4 bytes (n / 4 + 1 always suffice);
 * out[0] = l_pac, out[1] = contigs, out[2] = holes, out[3] = ambiguous bases, out[4..7] = cnt_fwd, out[8] = windows; contig_rows: five values
 * per contig (header text [begin, end) in the text, '\r's included; offset; length; holes), contig_cap rows; hole_rows: three per hole (offset,
 * length, byte), hole_cap rows.  A cap that is too small is ARX_E_TOO_LARGE and nothing is written.  Returns ARX_OK; ARX_E_OPEN for what
 * arx_index_build refuses (out[9] = 1: a base before the first '>', 2: no base); ARX_E_DEVICE without the GPU. */
int arx_selftest_fasta_pack(int32_t device, const uint8_t *text, int64_t n, int64_t window_bytes, uint8_t *pac, int64_t pac_cap, int64_t *out,
                            int64_t *contig_rows, int64_t contig_cap, int64_t *hole_rows, int64_t hole_cap);

/* Loads <prefix>.{bwt,sa,pac,ann,amb,alt} (files written by `bwa index`) into HBM of `device`; derives there, once, what the kernels use
 * beside the files' content: the Occ blocks re-packed for one popcount per count; the k-mer tables of the seeding passes (ARX_KMER_K /
 * ARX_KMER_FWD: up to 69 GB + 5.7 GB at GRCh38 size, never more than a third of the free memory); the WHOLE suffix array and its inverse,
 * 40 bits per entry (2 x 31 GB at GRCh38 size, when they take no more than half of what is free after the tables; ARX_TEXT_INDEX=0: never),
 * or else the suffix-array sample every 4th row (ARX_SA_DENSE).  arx_index_info says what was built.  ~5 s for GRCh38. */
int arx_open(const char *prefix, int device, arx_ctx **out);
void arx_close(arx_ctx *ctx); /* also frees the context's batches that are still alive: their handles are invalid afterwards */
const char *arx_last_error(arx_ctx *ctx);      /* ctx may be NULL after a failed arx_open */
const char *arx_backend(void);                 /* "hip:gfx950" for the product library */
/* info[0] symbols of the index (2 x l_pac); [1] K of the k-mer table of the third seeding pass (0: none); [2] deepest per-depth table of the
 * forward extensions (0: none); [3] rows per resident suffix-array entry (1: the whole array); [4] 1 if the inverse suffix array is resident
 * (text mode of the seeding passes); [5] bytes of device memory the index holds; [6], [7] reserved (0) */
int arx_index_info(arx_ctx *ctx, int64_t *info /* 8 */);
int arx_ctx_device(arx_ctx *ctx);               /* the device ordinal ctx was opened on (-1: ctx is NULL) */

/* Page-locks host memory the caller hands to arx_batch_create / arx_batch_reset (bases) or receives results in (arx_batch_fetch,
 * arx_batch_rfa_fetch, arx_batch_post_fetch), for as long as it keeps reusing those arrays: copies then run at PCIe speed without a
 * staging copy (the reference recycles its per-work-unit buffers the same way, aligner.go:234 ReturnBuffer, gobwa.go:107-126 Arena).
 * Optional: unregistered memory works, through the library's own staging.  Unregister before freeing.  ARX_E_ARG when the range cannot
 * be (un)registered (e.g. registered already). */
int arx_host_register(void *ptr, int64_t bytes);
int arx_host_unregister(void *ptr);

int arx_contigs(arx_ctx *ctx, int32_t *n, const char *const **names, const int64_t **offsets, const int32_t **lens,
                const int32_t **is_alt, int64_t *l_pac);

/* bases: concatenated reads as codes 0..4 (A,C,G,T,N); lens[n_reads]; read 2i and 2i+1 are mates (either may be empty).
 * Reads of one barcode are contiguous; barcode boundaries do not matter to this stage (pairs are independent). */
int arx_batch_create(arx_ctx *ctx, int32_t n_reads, const uint8_t *bases, const int32_t *lens, arx_batch **out);
/* Replaces the reads of an existing batch: same stream, same work memory, same input buffers when the new reads fit -- a caller in
 * steady state allocates nothing (what the reference does with its per-work-unit buffers: aligner.go:234 ReturnBuffer, gobwa.go:107-126
 * Arena).  Results of the previous run are gone; the uploads are asynchronous on the batch's stream (pinned staging inside). */
int arx_batch_reset(arx_ctx *ctx, arx_batch *b, int32_t n_reads, const uint8_t *bases, const int32_t *lens);
/* Runs the stages up to last_stage.  Stages already done are kept: run(ARX_STAGE_SEED) followed by run(ARX_STAGE_ALN) resumes after
 * seeding; asking for a stage that is already done (or an earlier one) restarts the batch from its reads.  All work memory of the
 * batch is reused by the next run, so results (arx_batch_fetch, arx_batch_rfa_fetch) must be fetched before it. */
int arx_batch_run(arx_ctx *ctx, arx_batch *b, int32_t last_stage);
/* counts[8] = n_reads, n_regs, n_cigar_words, seed occurrences, extension rounds, extension DPs, rescue rounds, rescue SWs */
int arx_batch_counts(arx_ctx *ctx, arx_batch *b, int64_t *counts);
/* ---- device-resident boundary (multi-GPU dataflow): a batch whose reads are in the memory of this context's GPU already
 * -- received from the ingest GPU over RCCL -- and result slabs handed out where they lie, for a send without a host copy.
 * arx_batch_reset_device: arx_batch_reset from device pointers (d_bases: n_bases codes 0..4; d_lens: n_reads lengths); the caller's
 * buffers must be complete when it is called and may be reused when it returns.  arx_batch_device_view: the dense result arrays of
 * arx_batch_fetch / arx_batch_rfa_fetch in device memory (cand_off / cands NULL before arx_batch_rfa); valid until the batch is run, reset
 * or freed; the call waits for the batch's stream.  (In the host test double "device" memory is host memory.) */
typedef struct {
	int64_t n_reads, n_regs, n_cigar, n_cands;
	const int32_t *reg_off; const arx_reg *regs; const arx_aln *alns; const uint32_t *cigars;
	const int32_t *cand_off; const struct arx_cand_ *cands;
} arx_device_view;
int arx_batch_reset_device(arx_ctx *ctx, arx_batch *b, int32_t n_reads, int64_t n_bases, const uint8_t *d_bases, const int32_t *d_lens);
int arx_batch_device_view(arx_ctx *ctx, arx_batch *b, arx_device_view *view);

/* reg_off[n_reads+1], regs[n_regs], alns[n_regs], cigars[n_cigar_words]: caller-allocated from arx_batch_counts */
int arx_batch_fetch(arx_ctx *ctx, arx_batch *b, int32_t *reg_off, arx_reg *regs, arx_aln *alns, uint32_t *cigars);
void arx_batch_free(arx_ctx *ctx, arx_batch *b);

/* ---- the Go half of the per-barcode path (src/aligner/aligner.go): candidates per read (GetChains :1633, GetAlignments :1484),
 * tagBestAlignments :1397, inferMolecules :1300 ... optimizer.Optimize (src/optimizer/optimizer.go:15) and estimateMapQualities :797.
 * Needs arx_batch_run(..., ARX_STAGE_ALN) first.  One candidate per region, or one placeholder (reg = -1, pos = -1) for a read
 * without regions; `active` marks the placement chosen for the read, `mapq` is set on active candidates. */
typedef struct arx_cand_ {
	int64_t pos, aend;              /* Alignment.pos / .aend (0-based, reverse-strand candidates swapped +1, aligner.go:1577-1582) */
	double sum_move;                /* 1 + sum of 10^fastScore over sink molecules (method 2) */
	int32_t reg, read, rid, reversed, score, mismatches, indels, soft_clipped, soft_clipped_length;
	int32_t lap2;                   /* log_alignment_probability * 2 */
	int32_t active, is_proper, mapq, molecule_id, active_molecule, in_filtered /* score >= best - 17 */, best_in_mol, pad;
} arx_cand;
/* bc_pair_off[n_barcodes+1]: pair offsets of the (whole) barcodes in the batch; do_rfa[b]: worthRunningRFA (aligner.go:1018-1030),
 * decided by the caller from the barcode string; penalty: the reference's -i flag (a float64, main.go:28; default -4).  Only integer
 * values are accepted (ARX_E_ARG with a message otherwise): every score term is then a multiple of 0.5 and the sums are exact in any
 * order, which is what makes the result well defined; cen_start/cen_end per contig or NULL. */
int arx_batch_rfa(arx_ctx *ctx, arx_batch *b, int32_t n_barcodes, const int64_t *bc_pair_off, const uint8_t *do_rfa, double penalty,
                  const int64_t *cen_start, const int64_t *cen_end, int64_t *n_cands);
int arx_batch_rfa_fetch(arx_ctx *ctx, arx_batch *b, int32_t *cand_off /* n_reads+1 */, arx_cand *cands /* n_cands */);

/* Overlapping the way home with the next super-batch (a worker with two host threads per handle).  arx_batch_detach copies the dense results of
 * the run -- and of arx_batch_rfa when it has run -- aside on the device (memory of the handle's own, outside its work memory; < 1 ms) and says
 * how large they are: sizes[0..3] = reads, regions, CIGAR words, candidates.  From then on the handle may be reset and run again by one thread
 * while ANOTHER thread calls arx_batch_fetch_detached, which copies them to host arrays on a stream of its own (any pointer may be NULL: not
 * wanted).  The next arx_batch_detach of the same handle must wait until that call has returned (the caller's ordering).  The reference's
 * workers overlap the same way: results of one work unit are written out while the next is aligned (aligner.go:335-371). */
int arx_batch_detach(arx_ctx *ctx, arx_batch *b, int64_t *sizes /* 4 */);
int arx_batch_fetch_detached(arx_ctx *ctx, arx_batch *b, int32_t *reg_off, arx_reg *regs, arx_aln *alns, uint32_t *cigars, int32_t *cand_off, arx_cand *cands);

/* ---- what the reference computes per barcode between placement and the BAM records, on the candidates arx_batch_rfa left on the
 * device (needs arx_batch_rfa first; uses its barcodes, penalty and centromeres):
 *   the CIGAR walk of GetAlignments (aligner.go:1505-1570, against GetSeq gobwa.go:50-80): matches and the mismatch locations in
 *   reference (contig) and read coordinates -- the host never re-fetches the reference; readmap_s/_e (gobwa.go:368-369);
 *   markDuplicates (aligner.go:611-641); CheckSplitReads / GetSplitAlignment (split.go:31-163). */
typedef struct {
	int32_t qb, qe;                 /* Alignment.readmap_s / readmap_e */
	int32_t matches;                /* Alignment.matches */
	int32_t n_mm, mm_off;           /* Alignment.mismatchLocs / mismatchReadLocs = mm_ref / mm_read[mm_off .. mm_off + n_mm) */
	int32_t duplicate;              /* Alignment.duplicate */
} arx_cand_post;
typedef struct {                    /* per read: Alignment.secondary of its active candidate */
	int32_t split;                  /* candidate index, -1 for none */
	int32_t mapq, is_proper;        /* split.mapq, split.is_proper */
	int32_t n_split_cand;           /* candidates that passed split.go:85-97 */
	int32_t order_pinned;           /* 0: > 12 such candidates with a score tie that decides the result -- Go's unstable sort.Sort picks there */
	int32_t second_best2, score2;   /* split.mapq_data.second_best_score * 2, .score * 2 */
	int32_t pad;
} arx_split;
int arx_batch_post(arx_ctx *ctx, arx_batch *b, int64_t *n_mm);
/* post[n_cands], split[n_reads], mm_ref[n_mm], mm_read[n_mm]; any of them may be NULL */
int arx_batch_post_fetch(arx_ctx *ctx, arx_batch *b, arx_cand_post *post, arx_split *split, int32_t *mm_ref, int32_t *mm_read);

/* ---- what estimateMapQualities leaves in mapq_data of every read's active alignment (aligner.go:847-889) and AppendBam writes as
 * XS / AS / XC / XM / XT / DM (bamwriter.go:390-460, 555-563), on the candidates arx_batch_rfa left on the device (needs arx_batch_rfa
 * first; a later arx_batch_rfa or arx_batch_post discards the result, so call it after arx_batch_post).  Not part of arx_batch_rfa: a
 * caller that writes no tags pays nothing.  second_best: the first non-active filtered candidate, in candidate order, whose best pair
 * score with the molecule term beats the running maximum (start -1000); xs = int(0.5 * its best pair score), or without one int(the
 * pseudo-count score of appendPsuedocountAlignmentScore, log_molecule_penalty included); as = int(0.5 * the pair score of the active
 * pair); integers truncated toward zero as Go's int() does.  dm_n / dm_sum: setMoleculeDifferences' inputs for the active candidate's
 * molecule (molecule_difference = dm_sum / dm_n). */
typedef struct {
	int32_t active;                 /* the read's active candidate (index into arx_batch_rfa_fetch's cands) */
	int32_t second_best;            /* mapq_data.second_best: candidate index, -1 for none */
	int32_t xs, as;                 /* int(mapq_data.second_best_score), int(mapq_data.score) */
	int32_t xm, xt;                 /* second_best.active_molecule; second_best.molecule_id == molecule_id (0 without a second best) */
	int32_t dm_n, dm_sum;           /* active alignments in the active candidate's molecule, sum of their mismatches (0, 0: no molecule) */
} arx_read_tags;
int arx_batch_tags(arx_ctx *ctx, arx_batch *b);
int arx_batch_tags_fetch(arx_ctx *ctx, arx_batch *b, arx_read_tags *out /* n_reads */);

/* ---- in front of the path: the reference's paired FASTQ reader (src/fastqreader/reader.go) re-shaped to deliver super-batches of
 * whole barcode sets -- what its producer loop (aligner.go:335-358) hands to one worker per set, one read pair per cgo call.
 * A set is what ReadBarcodeSet (reader.go:209-300) returns: consecutive records of one barcode, at most 30000, 201-record chunks
 * while a barcode continues across sets; `unique` is its third result (WorkUnit.unique_barcode), `do_rfa` = worthRunningRFA
 * (aligner.go:1018-1030).  bases/lens/set_pair_off/do_rfa go straight into arx_batch_create and arx_batch_rfa; the rest is what
 * the BAM records need.  Host code only: works without a GPU.  Pointers stay valid until the next call on the same feeder. */
typedef struct arx_feeder arx_feeder;
typedef struct {
	int32_t n_sets, pad;
	int64_t n_pairs;
	int64_t bad_lines;              /* lines skipped while looking for a record start (reader.go:156-159), since open */
	const int64_t *set_pair_off;    /* n_sets + 1 */
	const uint8_t *unique, *do_rfa; /* n_sets */
	const uint8_t *bases;           /* codes 0..4 (nst_nt4_table); read 2i / 2i+1 = Read1 / Read2 of pair i */
	const char *quals;              /* one byte per base, same layout */
	const int32_t *lens;            /* 2 * n_pairs */
	const uint8_t *valid;           /* n_pairs: FastQRecord.Valid (VX:i:1) */
	const int64_t *name_off; const char *names;       /* n_pairs + 1: FastQRecord.ReadInfo */
	const int64_t *rg_off; const char *rgs;           /* n_pairs + 1: FastQRecord.ReadGroupId */
	const int64_t *barcode_off; const char *barcodes; /* n_sets + 1: FastQRecord.Barcode of the set */
} arx_super_batch;
int arx_feeder_open(const char *r1_path, const char *r2_path, arx_feeder **out, char *msg, int32_t msg_cap); /* plain or gzip */
/* appends whole sets until at least target_pairs pairs are held (at least one set); returns the number of sets, 0 at the end of the
 * input, < 0 on a read error */
int arx_feeder_next(arx_feeder *f, int64_t target_pairs, arx_super_batch *out);
void arx_feeder_close(arx_feeder *f);
/* arx_feeder_open with the parse on ctx's GPU: two reader threads inflate the files side by side, HIP kernels find the lines, the records,
 * the header fields, the base codes and the barcode runs in the raw text.  chunk_bytes: bytes of each file's inflated stream per chunk (0: a
 * default of 8 MiB; at most 2^28); depth >= 1: super-batches whose arrays stay valid -- those of call k until call k + depth returns --, so
 * that one producer can feed `depth` workers.  arx_feeder_next / arx_feeder_close as for the host feeder; the arx_super_batch is byte for
 * byte the one arx_feeder_open's feeder delivers for the same files and target_pairs.  Needs the GPU (ARX_E_DEVICE without one; ARX_E_IO: a
 * file cannot be opened).  Two environment switches, read at open: ARX_FEEDER_PARSE_CHUNKS=n -- chunks of each file one parse takes in
 * (default: what fills 8 MiB, at most 64; 1 makes every chunk boundary a boundary between parses: what the tests use to put the carry
 * between parses at every byte offset; results do not depend on it); ARX_FEEDER_TIMES=1 -- diagnostics: arx_feeder_close prints the feeder
 * thread's seconds per stage and its kernels' times (HIP events) on stderr. */
int arx_feeder_open_device(arx_ctx *ctx, const char *r1_path, const char *r2_path, int64_t chunk_bytes, int32_t depth, arx_feeder **out, char *msg,
                           int32_t msg_cap);
/* arx_feeder_open_device with flags.  ARX_FEEDER_INFLATE_DEVICE: a file that is BGZF -- its first gzip member has an extra subfield BC of
 * length 2, the test htslib makes; what `samtools fastq -c` and bgzip write -- is read as it is and its blocks are inflated by a HIP kernel
 * (csrc/dev_inflate.h), one wavefront per block, straight into the text the parse kernels read: its reader thread only walks block headers,
 * and the upload is the compressed bytes.  R1 and R2 are looked at separately; a file that is anything else (plain text, ordinary gzip)
 * goes through zlib on its reader thread as without the flag.  chunk_bytes then counts inflated bytes of whole blocks: a chunk is the longest
 * run of blocks that inflate to at most chunk_bytes, at least one block.  A block that does not inflate (damaged stream, wrong CRC-32 or
 * ISIZE, a header that is not BGZF, a BSIZE that runs past the end of the file) ends the input in front of it like a read error of zlib
 * does: the sets that are complete are delivered, then arx_feeder_next returns < 0.  A missing EOF block is no error.  The super-batches
 * are byte for byte those of the plain text.  flags = 0 is arx_feeder_open_device exactly; unknown bits: ARX_E_ARG. */
#define ARX_FEEDER_INFLATE_DEVICE 1
/* ARX_FEEDER_GUNZIP_DEVICE (the bit of ARX_FQSORT_GUNZIP_DEVICE and ARX_FQSTD_GUNZIP_DEVICE): a file that is ordinary gzip -- the magic 1f 8b,
 * CM 8, and no BGZF block first -- is read as it is and inflated on the device in chunks (csrc/dev_gunzip.h, gunzip_host.h: one DEFLATE stream
 * per member, a wavefront per 32 KiB of it), a launch at a time, straight into the text the parse kernels read; the two files' launches are in
 * flight together, each on a stream of its own.  R1 and R2 are looked at separately; a BGZF file goes as without this flag (its kernel with
 * ARX_FEEDER_INFLATE_DEVICE, zlib without), plain text as ever.  For such a file a piece of text is what one launch accepts, and the feeder
 * asks for another while the file's window holds less than chunk_bytes; the compressed bytes per launch follow from chunk_bytes
 * (csrc/device_feeder.h states the rule).  Whatever the device does not take -- a refuted candidate, an overflow, a stored block in the way,
 * members cut short -- is inflated by zlib on the feeder's thread from there on; the device never declares a file bad.  Where zlib or a
 * member's trailer (CRC-32, ISIZE) reports an error the input ends there like at a read error: the sets that are complete are delivered, then
 * arx_feeder_next returns < 0.  The super-batches are byte for byte those of the plain text.  Two environment switches, read at open, for
 * tests: ARX_FEEDER_GUNZIP_CHUNK=n (compressed bytes per chunk) and ARX_FEEDER_GUNZIP_SLAB=n (per launch), within arx_selftest_gunzip's bounds
 * (ARX_E_ARG otherwise).  Off by default. */
#define ARX_FEEDER_GUNZIP_DEVICE 8
int arx_feeder_open_device_ex(arx_ctx *ctx, const char *r1_path, const char *r2_path, int64_t chunk_bytes, int32_t depth, int32_t flags, arx_feeder **out,
                              char *msg, int32_t msg_cap);
/* the reads of the super-batch the last arx_feeder_next delivered, in device memory, for arx_batch_reset_device (same validity as its host
 * arrays; the feeder's stream is done with them).  ARX_E_ARG for a host feeder or before the first super-batch. */
int arx_feeder_device_reads(arx_feeder *f, const uint8_t **d_bases, const int32_t **d_lens, int64_t *n_bases);
/* stats[8] of a device feeder since open: chunks read (both files), bytes of text that entered the parse (the same for the plain, gzip and
 * BGZF form of a text), records parsed, lines skipped, barcode runs, chunks that took a host fallback (always 0: a BGZF block has none, and what zlib
 * took over of a gzip file under ARX_FEEDER_GUNZIP_DEVICE is reported by arx_feeder_gunzip_stats), BGZF blocks inflated on the device, compressed
 * bytes uploaded for them (both 0 without ARX_FEEDER_INFLATE_DEVICE).  A gzip file's pieces count as chunks.  ARX_E_ARG for a host feeder. */
int arx_feeder_stats(arx_feeder *f, int64_t *stats);
/* stats[2 * ARX_GUNZIP_N_STATS] of a device feeder: for R1, then for R2, what the gzip inflate on the device has done so far, in the layout of
 * arx_selftest_gunzip's stats (launches, accepted chunks, the bytes zlib inflated, why it took over, ...).  All zero for a file the device was
 * not given (no ARX_FEEDER_GUNZIP_DEVICE, or not an ordinary gzip file).  ARX_E_ARG for a host feeder. */
int arx_feeder_gunzip_stats(arx_feeder *f, int64_t *stats);

/* ---- behind the path: the BAM sink.  The reference builds one biogo sam.Record per alignment on a single goroutine and
 * writes it twice (BamThread / AppendBams, src/aligner/bamwriter.go:615-627,279-282), two BGZF goroutines per writer (:118).  Here records
 * arrive in batches as flat arrays -- what AppendBam (:284-566) computes per alignment stays with the caller -- and are encoded and
 * BGZF-compressed on `threads` host threads, blocks written in order.  One arx_bam per output file (the barcode-sorted BAM, each position
 * bucket); host code only.  SAM/BAM specification v1 encoding; aux bytes are passed through as the caller encoded them. */
typedef struct arx_bam arx_bam;
typedef struct {
	int64_t n_records;
	const int64_t *name_off; const char *names;       /* n + 1 offsets; read names, 1..254 bytes each, no NUL */
	const int32_t *flag, *rid, *pos;                  /* rid = -1 and pos = -1 for an unmapped record (bamwriter.go:352-356) */
	const uint8_t *mapq;
	const int32_t *mate_rid, *mate_pos, *tlen;
	const int64_t *cigar_off; const uint32_t *cigars; /* BAM words: length << 4 | op, op in MIDNSHP=X = 0..8 */
	const int64_t *seq_off; const uint8_t *seq;       /* ASCII bases as written (already reverse-complemented where the caller does, :372-375) */
	const uint8_t *qual; int32_t qual_offset;         /* same offsets as seq; qual_offset is subtracted (33: fixQual, :240-247); 255: no qualities (0xff) */
	const int64_t *aux_off; const uint8_t *aux;       /* BAM-encoded aux fields of each record, back to back */
} arx_bam_batch;
/* extra_header: further header lines (e.g. @RG, @PG), each ending in '\n', or NULL; level: zlib 0..9 (-1: 6) */
int arx_bam_open(const char *path, int32_t n_contigs, const char *const *names, const int32_t *lens, const char *extra_header, int32_t threads, int32_t level,
                 arx_bam **out, char *msg, int32_t msg_cap);
int arx_bam_write(arx_bam *w, const arx_bam_batch *batch);
/* encodes and writes only records idx[0..n) of the batch, in that order (the position buckets of the reference's layout: every record
 * goes to the barcode-sorted BAM and to one bucket, bamwriter.go:279-281); the bytes of a record are those arx_bam_write writes for it */
int arx_bam_write_select(arx_bam *w, const arx_bam_batch *batch, const int64_t *idx, int64_t n);
/* stats[4] (may be NULL): records, BGZF blocks, uncompressed bytes, file bytes */
int arx_bam_close(arx_bam *w, int64_t *stats);
const char *arx_bam_error(arx_bam *w);
/* arx_bam_open whose BGZF blocks are compressed and checksummed on ctx's GPU (csrc/dev_bgzf.h, hip_bgzf.h): records are still encoded on
 * `threads` host threads; the stream is cut into blocks exactly where arx_bam_open's writer cuts it (every 65280 bytes; the header ends
 * its own block, the last block is partial, then the 28-byte EOF block) and every block goes through HIP kernels that produce a raw
 * DEFLATE stream -- greedy LZ77 parse, a length-limited dynamic Huffman code per block, or the fixed code or a stored block where that
 * is smaller: the size is known before a byte is written -- and the CRC-32 of the input, framed on the device and written in order.
 * After inflation the file is byte for byte arx_bam_open's; the compressed bytes are a function of the block's input only (not of batch
 * sizes, `threads`, the other blocks of a launch or the run).  There is no level.  The writers of one device share one set of streams, page-locked staging and
 * device buffers (about 64 MB and 100 MB), allocated by the first of them and kept until the process ends; their flushes take turns.  arx_bam_write, arx_bam_write_select, arx_bam_close (stats as above) and arx_bam_error take the handle as
 * they take arx_bam_open's.  ARX_E_ARG: ctx is NULL; ARX_E_IO: the file cannot be written; ARX_E_DEVICE: no GPU, or a HIP error (msg
 * says which; after open such errors surface as ARX_E_IO of the call with the text in arx_bam_error).  Never aborts. */
int arx_bam_open_device(arx_ctx *ctx, const char *path, int32_t n_contigs, const char *const *names, const int32_t *lens, const char *extra_header,
                        int32_t threads, arx_bam **out, char *msg, int32_t msg_cap);

/* Appends records that are BAM-encoded already -- block_size and all, as arx_batch_records writes them (csrc/dev_records.h; the bytes
 * BamSink::encode, csrc/bam_sink.h, produces for arx_bam_write) -- to a writer of either kind: n_bytes bytes holding exactly n_records records.
 * Only what is cheap is checked: the block_size fields must tile n_bytes into n_records records of at least 36 bytes; otherwise ARX_E_ARG and
 * nothing is appended.  May be mixed freely with arx_bam_write / arx_bam_write_select on one writer (AppendBams' order of calls is the file's
 * order of records, bamwriter.go:279-282). */
int arx_bam_write_encoded(arx_bam *w, const uint8_t *stream, int64_t n_bytes, int64_t n_records);
/* The same from DEVICE memory, for a writer of arx_bam_open_device only (ARX_E_ARG for arx_bam_open's): the stream never visits the host.  What
 * is compressed is the writer's carry (the bytes its last call left short of a block, fewer than 65280) followed by d_stream, cut every 65280
 * bytes as always; the carry goes up, the stream is copied device to device into the compressor's input, the kernels, framing and write order
 * are arx_bam_open_device's.  The tail short of a block comes home into the carry, so host and device writes interleave freely and
 * arx_bam_close is unchanged.  The block_size chain is not walked (it is in device memory): n_records is taken on trust for the statistics.
 * Ordering rule: d_stream must be COMPLETE when this is called -- arx_batch_records ends with its stream synchronised, as every phase does, so
 * a pointer from arx_batch_records_view qualifies -- and must stay valid until the call returns; it returns when its blocks are written, after
 * which the batch may be reset. */
int arx_bam_write_encoded_device(arx_bam *w, const uint8_t *d_stream, int64_t n_bytes, int64_t n_records);

/* ---- behind the sink: one coordinate-sorted BAM from the position buckets.  The reference writes the buckets so that each can be sorted in
 * memory and the results concatenated in file order (its -p flag, "to speed up final BAM concatenation"); it contains no sort itself.
 *
 * arx_bam_open_ex: ctx == NULL: arx_bam_open; otherwise arx_bam_open_device on ctx's GPU, and `level` is ignored.  flags bit 0,
 * ARX_BAM_COORDINATE: @HD says SO:coordinate instead of SO:unknown -- the order of what is appended stays the caller's business.  flags = 0
 * gives byte for byte the file of the call it stands for; any other bit: ARX_E_ARG. */
enum { ARX_BAM_COORDINATE = 1 };
int arx_bam_open_ex(arx_ctx *ctx, const char *path, int32_t n_contigs, const char *const *names, const int32_t *lens, const char *extra_header, int32_t threads,
                    int32_t level, int32_t flags, arx_bam **out, char *msg, int32_t msg_cap);
/* Appends the records of the BAM file in_path to the open writer w, on ctx's GPU (csrc/dev_bamsort.h, hip_bamsort.h): the file's BGZF blocks are
 * inflated there, the record starts found by segments walked side by side and verified against one another (exact whatever the data looks
 * like), and
 *   ARX_SORT_COORDINATE  the records are ordered stably by ((uint32_t)refID, pos) -- the SAM specification's SO:coordinate: refID = -1 last,
 *                        equal keys in file order, the strand no part of the key -- by a radix sort of (key, index) and a gather.  The whole
 *                        file is held at once, about 2.3 times its inflated size; a file that inflates to more than max_bytes (0: no limit
 *                        of its own) or whose working set exceeds the free device memory is ARX_E_TOO_LARGE, and msg names the remedy: a
 *                        smaller position bucket.  A refID outside [0, n_ref) sorts with -1
 *   ARX_SORT_COPY        the records are appended in file order, in slabs of whole BGZF blocks that inflate to at most max_bytes (0: 256 MiB;
 *                        at least one block) -- for a file that is its own sorted form, such as the unmapped bucket (refID = pos = -1
 *                        throughout).  Only a slab is in device memory; the compressed file is read into host memory whole.  The records
 *                        are counted by the same discovery, the chain carried from slab to slab
 * and the stream is handed to the writer: in device memory to a writer of ctx's device (arx_bam_write_encoded_device's path), fetched to a host
 * writer.  mode | ARX_SORT_TIMED waits for every launch and fills the phase times of stats.  ARX_E_ARG: the input's header does not list
 * exactly the context's contigs (count, names, lengths), or bad arguments; ARX_E_IO, nothing appended: the file cannot be read, is not BGZF, a
 * block does not inflate, it has no BAM header, or the chain of block_size fields breaks or does not end with the stream -- or the writer
 * failed (then its arx_bam_error has the text too); ARX_E_DEVICE: a HIP error.  msg (may be NULL) receives the text.
 * stats[20] (may be NULL): [0] records appended, [1] inflated bytes, [2] BGZF blocks, [3] segments, [4] segments whose guess was right,
 * [5] segments repaired, [6] repair rounds, [7] slabs; microseconds: [8] read and header, [9] upload and inflate, [16] compress and write,
 * [17] the call; with ARX_SORT_TIMED also [10] probe, [11] walk and fill, [12] verify and repair, [13] keys, [14] key sort, [15] sizes, scan
 * and gather. */
enum { ARX_SORT_COORDINATE = 0, ARX_SORT_COPY = 1, ARX_SORT_TIMED = 0x100 };
int arx_bam_sort_append(arx_ctx *ctx, arx_bam *w, const char *in_path, int32_t mode, int64_t max_bytes, int64_t *stats, char *msg, int32_t msg_cap);
/* self-test of the discovery, key, sort and gather kernels on plain record bytes, no index and no file needed (tests/test_bam_sort_gpu.py):
 * stream[0..n_bytes) is a chain of BAM records from its first byte, n_ref what the probe holds refID against, seg_bytes the segment size (a
 * power of two, at least 64; arx_bam_sort_append uses 256 KiB).  out[n_bytes] receives the records in coordinate order (mode ARX_SORT_COPY: as
 * they are), rec_off[*n_records + 1] where they start in out (room for n_bytes / 36 + 2 entries always suffices).  ARX_E_IO: the chain is
 * broken; out and rec_off are untouched.  stats[20] (may be NULL) as above, without blocks and file times. */
int arx_selftest_bam_sort(int32_t device, const uint8_t *stream, int64_t n_bytes, int32_t n_ref, int64_t seg_bytes, int32_t mode, uint8_t *out, int64_t *rec_off,
                          int64_t *n_records, int64_t *stats);

/* ---- beside the final BAM: its .bai (the SAM specification, 5.2), built on the GPU (csrc/dev_bamindex.h, hip_bamindex.h).  device: a HIP
 * device index -- no context is needed, the contigs are the BAM header's own.  The file must be sorted by coordinate, as arx_bam_sort_append
 * leaves it.  Its BGZF blocks are inflated on the device in slabs of whole blocks that inflate to at most max_bytes (0: 256 MiB; at least one
 * block), the record starts found by the sort's discovery, and every record indexed by one lane.  The contract:
 *   virtual offsets  the file's blocks are b = 0 .. nb-1; at[b] is a block's file offset, ooff[b] where its bytes start in the inflated stream,
 *             isize[b] its inflated size.  For an inflated offset o < total, b is the one block with ooff[b] <= o < ooff[b] + isize[b] (empty
 *             blocks hold nothing) and V(o) = at[b] << 16 | (o - ooff[b]).  V(total) = at[b'] << 16 with b' the first block behind the last
 *             non-empty one (normally the EOF block), or the file size where there is none.  A record that starts at o and is followed by one
 *             at o' occupies [V(o), V(o')); the last record ends at V(total).  at must stay below 2^48
 *   interval  beg = pos; end = pos + 1 where flag bit 4 is set, n_cigar_op is 0 or the operations consume no reference, otherwise pos + the
 *             summed lengths of the operations M, D, N, = and X (0, 2, 3, 7, 8); bin = reg2bin(beg, end) as the specification's 5.3 states it.
 *             The record's own bin field is not read, and the CG-tag form of CIGARs above 65,535 operations is not interpreted
 *   chunks    in file order a run is a maximal sequence of consecutive records with the same (refID, bin), from its first record's begin to
 *             its last record's end; the runs of one bin, in file order, are its chunks; two neighbouring chunks are joined when
 *             (earlier.end >> 16) >= (later.beg >> 16) -- a reader that has reached the block where the earlier ends gains nothing from a
 *             seek.  Bins are written in ascending order of their number.  htslib's folding of small bins into their parents is NOT done
 *             (the index is valid without it): byte equality with `samtools index` is not claimed and was never checked
 *   pseudo-bin 37450  last in every contig that holds a record: (V(first record), end of the last record) and (records without flag bit 4,
 *             records with it)
 *   linear    windows of 16,384 bases; a record sets the windows beg >> 14 .. (end - 1) >> 14; a window's value is the smallest V(start) among
 *             the records that set it; n_intv = 1 + the highest window set in the contig; an unset window below that takes the value of the
 *             next set window above it.  A contig without records has n_bin = 0 and n_intv = 0
 *   trailer   n_no_coor, the number of records with refID = -1, is always written
 * Refused, with nothing written and no partial file left (the index is written as <bai>.tmp and renamed at the end):
 *   ARX_E_ARG  msg names the record (numbered from 0 in file order) and the rule: the keys ((uint32_t)refID, pos) are not non-decreasing, also
 *             across a slab border; a refID outside [-1, n_ref); refID >= 0 with pos < 0; an end beyond the record's contig length.  Also: a
 *             contig longer than 2^29, the BAI format's limit (the CSI index of such a file is arx_bam_index_csi's to write); a file of 2^48
 *             bytes or more; unknown flag bits
 *   ARX_E_IO  the file is unreadable or not BGZF, a block does not inflate, there is no BAM header, the chain of block_size fields breaks or
 *             does not end with the stream, a record's name and CIGAR do not fit into its block_size, or the index cannot be written
 *   ARX_E_DEVICE  there is no such device, or a HIP error: there is no CPU fallback.  ARX_E_TOO_LARGE: a slab does not fit the device memory
 * stats[20] (may be NULL): [0] records, [1] inflated bytes, [2] BGZF blocks, [3] slabs, [4] runs of records with a refID, [5] chunks written,
 * [6] bins written without the pseudo-bins, [7] linear entries written, [8] n_no_coor; microseconds: [10] read and header, [11] upload and
 * inflate, [15] serialise and write, [16] the call; with ARX_BAI_TIMED, which waits for every launch, also [12] discovery, [13] the record
 * kernels, [14] run scans, sort and merge (with the fetch of the chunks). */
enum { ARX_BAI_TIMED = 0x100 };
int arx_bam_index(int32_t device, const char *bam_path, const char *bai_path /* NULL: bam_path + ".bai" */,
                  int64_t max_bytes /* inflated bytes of a slab; 0: 256 MiB */, int32_t flags /* ARX_BAI_TIMED or 0 */,
                  int64_t *stats /* [20], may be NULL */, char *msg, int32_t msg_cap);
/* self-test of the same indexing on an inflated stream in host memory, no file needed (tests/test_bam_index_gpu.py): stream[0..n_bytes) is the
 * BAM's inflated bytes, records from hdr on; the contigs; the block table the virtual offsets are made of (blk_at: n_blocks + 1 file offsets,
 * the last the file's size; blk_isize sums to n_bytes); seg_bytes: the discovery's segment (a power of two, at least 64); slab_bytes: the
 * inflated bytes of a slab (0: one slab; otherwise whole blocks, at least one).  out[0..*out_len) receives the .bai's bytes (ARX_E_TOO_LARGE:
 * out_cap is too small).  Codes as above, without a text; on a refusal by a record rule stats[9] is the record's number << 8 | the rule
 * (1 fields, 2 refID, 3 pos, 4 end, 5 order). */
int arx_selftest_bam_index(int32_t device, const uint8_t *stream, int64_t n_bytes, int64_t hdr,
                  int32_t n_ref, const int32_t *ref_len,
                  int64_t n_blocks, const int64_t *blk_at /* n_blocks + 1 file offsets */, const int32_t *blk_isize /* sum = n_bytes */,
                  int64_t seg_bytes, int64_t slab_bytes, uint8_t *out, int64_t out_cap, int64_t *out_len, int64_t *stats);

/* ---- the same file's .csi (CSIv1, the companion of the SAM specification), for contigs of up to 2^31 - 1 bases: a sibling of arx_bam_index on
 * the same device machinery (the functors of csrc/dev_bamindex.h carry the bin scheme as a value; the BAI is the scheme (14, 5)).  device, the
 * sorted file, the slabs of max_bytes, the discovery and the lane per record are arx_bam_index's.  The contract:
 *   virtual offsets  the file's blocks are b = 0 .. nb-1; at[b] is a block's file offset, ooff[b] where its bytes start in the inflated stream,
 *             isize[b] its inflated size.  For an inflated offset o < total, b is the one block with ooff[b] <= o < ooff[b] + isize[b] (empty
 *             blocks hold nothing) and V(o) = at[b] << 16 | (o - ooff[b]).  V(total) = at[b'] << 16 with b' the first block behind the last
 *             non-empty one (normally the EOF block), or the file size where there is none.  A record that starts at o and is followed by one
 *             at o' occupies [V(o), V(o')); the last record ends at V(total).  at must stay below 2^48
 *   scheme    min_shift lies in [10, 24], 0 means 14, anything else is ARX_E_ARG.  depth is the smallest d >= 5 with 2^(min_shift + 3 d) >= the
 *             longest contig of the header.  Every contig length up to 2^31 - 1 is accepted, so depth <= 7 and every bin number is below 2^22.
 *             At min_shift 14 a header whose contigs are all <= 2^29 gives depth 5, the BAI's scheme; one contig of 2^29 + 1 gives depth 6.
 *             The depth is never below the BAI's 5, whatever the contigs.  htslib adds 256 to the length before it chooses the depth and starts
 *             from depth 0; we do neither: byte equality with `samtools index -c` is not claimed and was never checked
 *   interval  beg = pos; end = pos + 1 where flag bit 4 is set, n_cigar_op is 0 or the operations consume no reference, otherwise pos + the
 *             summed lengths of the operations M, D, N, = and X (0, 2, 3, 7, 8).  The record's own bin field is not read, and the CG-tag form
 *             of CIGARs above 65,535 operations is not interpreted
 *   bin       the first bin of level l is (8^l - 1) / 7.  bin(beg, end) is the deepest level l <= depth at which beg and end - 1 share
 *             >> (min_shift + 3 (depth - l)), plus that shifted value; it is bin 0 where none does.  At (14, 5) this is the specification's
 *             reg2bin (5.3) value for value
 *   chunks    in file order a run is a maximal sequence of consecutive records with the same (refID, bin), from its first record's begin to
 *             its last record's end; the runs of one bin, in file order, are its chunks; two neighbouring chunks are joined when
 *             (earlier.end >> 16) >= (later.beg >> 16).  Bins are written in ascending order of their number.  htslib's folding of small bins
 *             into their parents is NOT done
 *   loffset   one table of windows of 2^min_shift bases per contig; a record sets the windows beg >> min_shift .. (end - 1) >> min_shift; a
 *             window's value is the smallest V(start) among the records that set it; an unset window below the highest set one takes the
 *             value of the next set window above it (the BAI's linear index at another window size).  A bin's loffset is the value of the
 *             first window of the bin's interval, which is never above the highest set one: a record of the bin sets a window at or behind
 *             it.  This is htslib's rule (update_loff), a valid lower bound for a reader that walks from the leaf bin of beg to earlier
 *             siblings and parents until a bin exists, because the table does not decrease in a sorted file
 *   meta-bin  number (8^(depth+1) - 1) / 7 + 1 -- 37450 at depth 5, 299594 at depth 6, 2396746 at depth 7 --, last in every contig that holds
 *             a record, loffset 0, two chunks: (V(first record), end of the last record) and (records without flag bit 4, records with it)
 *   bytes     "CSI\1", min_shift, depth, l_aux = 0, n_ref (int32 each); per contig n_bin; per bin: bin (uint32), loffset (uint64), n_chunk
 *             (int32), the chunks (two uint64 each); then n_no_coor (uint64), always written.  A contig without records has n_bin = 0.  There
 *             is no linear index and no tabix aux block in the file
 *   file      those bytes as BGZF: blocks of at most 65,280 input bytes, the 28-byte EOF block last, compressed on the host by zlib (the host
 *             sink's code).  The inflated bytes are what this contract pins; the compressed ones are not
 * Refused, with nothing written and no partial file left (the index is written as <csi>.tmp and renamed at the end):
 *   ARX_E_ARG  msg names the record (numbered from 0 in file order) and the rule: the keys ((uint32_t)refID, pos) are not non-decreasing, also
 *             across a slab border; a refID outside [-1, n_ref); refID >= 0 with pos < 0; an end beyond the record's contig length.  Also: a
 *             min_shift outside [10, 24] that is not 0; a file of 2^48 bytes or more; unknown flag bits
 *   ARX_E_IO  the file is unreadable or not BGZF, a block does not inflate, there is no BAM header, the chain of block_size fields breaks or
 *             does not end with the stream, a record's name and CIGAR do not fit into its block_size, or the index cannot be written
 *   ARX_E_DEVICE  there is no such device, or a HIP error: there is no CPU fallback.  ARX_E_TOO_LARGE: a slab does not fit the device memory
 * stats[20] (may be NULL) as arx_bam_index's, except: [7] the depth chosen, [17] min_shift as used. */
int arx_bam_index_csi(int32_t device, const char *bam_path, const char *csi_path /* NULL: bam_path + ".csi" */, int32_t min_shift /* 0: 14 */,
                  int64_t max_bytes /* inflated bytes of a slab; 0: 256 MiB */, int32_t flags /* ARX_BAI_TIMED or 0 */,
                  int64_t *stats /* [20], may be NULL */, char *msg, int32_t msg_cap);
/* self-test of the same indexing on an inflated stream in host memory (tests/test_bam_index_csi_gpu.py): arx_selftest_bam_index's arguments,
 * with min_shift behind slab_bytes.  out[0..*out_len) receives the INFLATED bytes of the .csi, which arx_bam_index_csi compresses
 * (ARX_E_TOO_LARGE: out_cap is too small, nothing is written).  Codes as above, without a text; on a refusal by a record rule stats[9] is
 * the record's number << 8 | the rule (1 fields, 2 refID, 3 pos, 4 end, 5 order). */
int arx_selftest_bam_index_csi(int32_t device, const uint8_t *stream, int64_t n_bytes, int64_t hdr,
                  int32_t n_ref, const int32_t *ref_len,
                  int64_t n_blocks, const int64_t *blk_at /* n_blocks + 1 file offsets */, const int32_t *blk_isize /* sum = n_bytes */,
                  int64_t seg_bytes, int64_t slab_bytes, int32_t min_shift, uint8_t *out, int64_t out_cap, int64_t *out_len, int64_t *stats);

/* ---- the index written by the writer itself, while it appends: an opt-in coordinate writer that builds the .bai or the .csi of what it is
 * given on ctx's GPU as the bytes pass through it, and writes the index when it is closed -- no second pass reads the file back.  The one rule:
 * for every sequence of appends the writer accepts, the BAM is byte for byte the file the same appends give a writer without an index, and the
 * index's bytes (the .csi's inflated ones) are exactly those arx_bam_index or arx_bam_index_csi (same min_shift) writes for that finished file:
 * virtual offsets, interval, chunks and their join rule, pseudo-bin or meta-bin, linear table or loffset and trailer are stated there.
 *   how       a writer's layout is known before any compressed size is: the header ends its own ceil(H / 65280) blocks, every block behind
 *             holds 65280 bytes of the record stream but the last.  The kernels of arx_bam_index run on block ordinal << 16 | offset within in
 *             place of V (the two order alike, and the join rule decides alike); the sink records the file offset of every block it writes (8
 *             bytes a block), and the close turns the one into the other by a lookup.  What is appended from device memory
 *             (arx_bam_sort_append in both modes, arx_bam_write_encoded_device) is indexed where it lies; what comes from the host
 *             (arx_bam_write, arx_bam_write_select, arx_bam_write_encoded) is uploaded in pieces for it.  Device memory: the window table for
 *             the writer's life, and per append one piece of at most 256 MiB of its bytes with 56 bytes per record and about 100 per run
 *   open      arx_bam_open_ex's arguments; ctx is required.  flags: ARX_BAM_COORDINATE is implied; ARX_BAM_DEVICE_SINK compresses the blocks
 *             on ctx's GPU (arx_bam_open_device; `level` is ignored), otherwise by zlib on the host.  index: ARX_BAM_INDEX_BAI, _CSI, or _AUTO
 *             (the .csi where a contig is longer than 2^29, else the .bai); min_shift as arx_bam_index_csi's (read for a .csi only);
 *             index_path NULL: path + ".bai" or ".csi".  ARX_E_ARG: a null ctx, unknown flag bits or index, a min_shift outside [10, 24] that is
 *             not 0, or ARX_BAM_INDEX_BAI with a contig longer than 2^29 (msg names it); nothing is created then
 *   appends   index first, then append.  An append that a record rule refuses -- the keys not non-decreasing, also across appends; a refID
 *             outside [-1, n_ref); pos < 0 with a refID; an end beyond the contig -- appends nothing and returns ARX_E_ARG; the text
 *             (arx_bam_error, or msg of arx_bam_sort_append) names the record, numbered from 0 over everything the writer has taken, and the rule.
 *             (arx_bam_sort_append in copy mode hands a file over slab by slab: the slabs in front of the refused one are in the file.)  A
 *             record whose name and CIGAR do not fit its block_size is ARX_E_IO.  The index is all or nothing: after a refused append the
 *             writer goes on as a plain BAM writer.  arx_bam_sort_append with a ctx on another device than the writer's: ARX_E_ARG
 *   close     arx_bam_close_indexed: stats as arx_bam_close's; index_stats[20] (may be NULL) as arx_bam_index's, the read and inflate times 0,
 *             [15] serialise and write, [16] the time spent indexing, appends and close together ([12] .. [14] stay 0).
 *             The index is written as <index>.tmp and renamed after the BAM has closed.  After a refused append: no index and no .tmp, and
 *             ARX_E_ARG with a text that says that the BAM is complete and the index was not written.  ARX_E_IO: the BAM or the index cannot be
 *             written, or the record stream ends inside a record.  arx_bam_close on such a writer does the same without the outputs; and
 *             arx_bam_close_indexed on a plain writer is arx_bam_close. */
enum { ARX_BAM_DEVICE_SINK = 2 };
enum { ARX_BAM_INDEX_BAI = 1, ARX_BAM_INDEX_CSI = 2, ARX_BAM_INDEX_AUTO = 3 };
int arx_bam_open_indexed(arx_ctx *ctx, const char *path, int32_t n_contigs, const char *const *names, const int32_t *lens, const char *extra_header, int32_t threads,
                         int32_t level, int32_t flags, int32_t index, int32_t min_shift /* 0: 14 */, const char *index_path /* NULL: path + ".bai" / ".csi" */,
                         arx_bam **out, char *msg, int32_t msg_cap);
int arx_bam_close_indexed(arx_bam *w, int64_t *stats /* [4], may be NULL */, int64_t *index_stats /* [20], may be NULL */, char *msg, int32_t msg_cap);
/* self-test of that indexing without files (tests/test_bam_index_feeds_gpu.py): arx_selftest_bam_index's stream, hdr, contigs and seg_bytes; the
 * record stream behind hdr is fed in n_feeds feeds that end at the stream's offsets feed_end[] (ascending, anywhere -- an end inside the header
 * feeds nothing --, the last n_bytes), every feed indexed in pieces of at most piece_bytes (0: whole); blk_at[n_blocks + 1] are the file offsets
 * of the writer's layout (strictly ascending, the last the EOF block's; n_blocks must be ceil(hdr / 65280) + ceil((n_bytes - hdr) / 65280), else
 * ARX_E_ARG); min_shift -1: the .bai, else the .csi's.  out, the codes and stats as the two self-tests above; a stream that ends inside a record
 * is ARX_E_IO. */
int arx_selftest_bam_index_feeds(int32_t device, const uint8_t *stream, int64_t n_bytes, int64_t hdr, int32_t n_ref, const int32_t *ref_len, int64_t n_blocks,
                                 const int64_t *blk_at, int64_t seg_bytes, int64_t n_feeds, const int64_t *feed_end, int64_t piece_bytes, int32_t min_shift, uint8_t *out,
                                 int64_t out_cap, int64_t *out_len, int64_t *stats);

/* ---- in front of the feeder: a FASTQ file pair sorted by barcode on the GPU -- the reference's `arachne preprocess`
 * (src/preprocess/preprocess.go:42-114: samtools import -T '*' | samtools sort -t BX | samtools fastq -T '*'), which the aligner needs: the
 * feeder opens a new barcode set wherever the barcode changes, so a barcode that returns later in the file would be placed as several
 * molecules.  The contract:
 *   record    what the feeder recognises.  Lines exist only where they end in '\n'; the lines of R1 and R2 are walked in lockstep up to the
 *             shorter file's line count; while searching, a pair whose R1 line is non-empty and starts with '@' opens a record of four line
 *             pairs, any other pair is skipped; a record that the end of either file cuts off does not exist
 *   barcode   the feeder's: the value of the leftmost BX:Z:(\S+)\s of the R1 header, the header's own newline closing a value, white space
 *             being ' ', \t, \n, \r, \v, \f; no match: the empty barcode.  R2's header plays no part
 *   output    every record's eight lines verbatim, four to each output file, ordered by barcode as unsigned bytes (byte-wise, a proper prefix
 *             first: strcmp's order extended to any byte, so the empty barcode comes first, as `samtools sort -t` puts records without the
 *             tag), equal barcodes in input order (stable, as samtools' merge sort).  Skipped lines and the cut-off record are dropped
 * So the feeder sees every barcode of the output as exactly one run, and the records it delivers are the input's.  The output is not the
 * bytes of the samtools pipeline, which rewrites the headers (tab-separated tags, /1 and /2).
 * device: a HIP device index -- no context is needed, and none should be open beside a large sort: its index competes for the memory.
 * Inputs may be plain text, gzip or BGZF, each file judged by itself; a BGZF file is inflated on the device.  Outputs are plain text, or
 * with ARX_FQSORT_BGZF BGZF files (blocks cut every 65280 bytes, the 28-byte EOF block last) that inflate to the same bytes; they are
 * written as <path>.tmp and renamed at the end: a failing call leaves nothing behind.  ARX_FQSORT_GUNZIP_DEVICE: an input that is an ordinary gzip
 * file (not BGZF) is inflated on the device in chunks (csrc/dev_gunzip.h) instead of by zlib on a reader thread; the same bytes come out, and a
 * file on which zlib's gzread reports an error is ARX_E_IO as without the flag.  ARX_FQSORT_CHECK: nothing is written, the output
 * paths may be NULL, only stats is filled -- stats[6] == stats[7] says that the input needs no sort.  ARX_FQSORT_TIMED waits for every
 * launch and books the phases per launch group.  Both texts and 80 bytes per record stay in device memory (csrc/hip_fqsort.h); max_bytes
 * (0: no limit of its own) bounds the inflated bytes of both files together.  ARX_E_TOO_LARGE: more than max_bytes, or than the device
 * holds -- msg names the remedy: sort per lane, or split the input (arx_fastq_sort_ex below sorts such a pair in runs); ARX_E_IO: a file cannot be read or
 * written, or a block does not inflate (nothing is produced then, where the feeder delivers the sets in front of the damage); ARX_E_ARG:
 * null paths without CHECK, unknown flag bits, an output path that is an input; ARX_E_DEVICE: no GPU, or a HIP error.
 * stats[20] (may be NULL): [0] records written, [1] [2] inflated bytes read from R1, R2, [3] [4] bytes written to R1, R2 as inflated text,
 * [5] lines skipped, [6] barcode runs in the input, [7] distinct barcodes, [8] longest barcode, [9] sort passes, [10] parse windows,
 * [11] output slabs, then microseconds: [12] waiting for the readers, [13] upload and inflate, [14] parse, [15] keys (TIMED only: otherwise
 * under [16]), [16] sort passes, [17] gather, [18] compress and write of BGZF blocks, [19] fetch and write of plain text, last blocks, rename */
enum { ARX_FQSORT_BGZF = 1, ARX_FQSORT_CHECK = 2, ARX_FQSORT_GUNZIP_DEVICE = 8, ARX_FQSORT_TIMED = 0x100 };
int arx_fastq_sort(int32_t device, const char *r1_in, const char *r2_in, const char *r1_out, const char *r2_out, int32_t flags, int64_t max_bytes, int64_t *stats,
                   char *msg, int32_t msg_cap);
/* self-test of the same orchestration (preprocess.go:42-114 as above) on two texts in host memory, no file and no index needed
 * (tests/test_fastq_sort_gpu.py).  window_bytes: the text a parse looks at per file (0: the 32 MiB of arx_fastq_sort; otherwise at least 128
 * and at most 2^29 -- ARX_E_ARG outside; a line or record that a window does not hold is ARX_E_TOO_LARGE); slab_bytes: the output bytes per
 * file that are gathered at a time (0: 64 MiB; a slab holds one record at least).  out1[n1], out2[n2] receive the sorted texts, out_len[2] their
 * lengths, rec_off1 / rec_off2[*n_records + 1] where the sorted records start (room for n1 / 5 + 2 entries always suffices), stats[20] (may
 * be NULL) as above.  On any error out1, out2, rec_off1 and rec_off2 are untouched. */
int arx_selftest_fastq_sort(int32_t device, const uint8_t *t1, int64_t n1, const uint8_t *t2, int64_t n2, int64_t window_bytes, int64_t slab_bytes, uint8_t *out1,
                            uint8_t *out2, int64_t *out_len, int64_t *rec_off1, int64_t *rec_off2, int64_t *n_records, int64_t *stats);
/* ---- the same sort of a file pair that device memory does not hold: sorted runs in temporary files, merged on the GPU.  The record, barcode
 * and output rules are arx_fastq_sort's, word for word; the output bytes do not depend on run_bytes, nor on how the readers cut their slabs,
 * and are arx_fastq_sort's for every input that call accepts.  flags, max_bytes (which here is what keeps a call from filling the disk),
 * msg and stats[0..19] as there; stats[6] is the input's own count of barcode runs.
 *   run_bytes == 0   exactly arx_fastq_sort: tmp_dir is ignored, stats[20..23] are 0
 *   run_bytes > 0    the inflated text of EACH file that one run holds in device memory, what the run before left over included; at least 128,
 *                    the smallest parse window (ARX_E_ARG below).  A run is parsed in windows of min(run_bytes, 32 MiB)
 *   run_bytes == -1  the library chooses: an eighth of the device memory that is free at the call less 1 GiB, in whole MiB, at least 32 MiB
 *                    and at most 16 GiB.  The accounting behind it: a run needs its two buffers (2 run_bytes), the readers' two slab texts
 *                    (64 MiB), the parse's windows and line index (about 128 MiB), four slab buffers (256 MiB) and a run's own 80 bytes per
 *                    record -- 1.6 run_bytes at 100 bytes of text per record and file --, which leaves about half of the free memory to what
 *                    grows with the whole input: 40 bytes and the barcode per record throughout, 40 bytes more per record while the merge
 *                    orders.  Nobody has measured which run size is fastest; fewer, larger runs mean fewer ranges per output slab.
 * Every record of a run is read, ordered and appended to the temporary files; the GPU keeps a table row and the barcode per record, orders
 * all rows at the end (stable: equal barcodes in run order, which is input order) and gathers the output slab by slab from the ranges of
 * the runs that the host reads back -- every temporary byte is written once and read once.
 * Temporary files: plain text, one per input file (arx_fqsort_XXXXXX.r1 / .r2, the name unique per call), under tmp_dir (NULL: the directory
 * of r1_out); the disk needed is the inflated size of both files; they are removed on every way out.  With ARX_FQSORT_CHECK no temporary
 * file is written and tmp_dir is not looked at: only the keys are kept, so an input of any size can be judged.  ARX_FQSORT_GUNZIP_DEVICE as
 * in arx_fastq_sort: a gzip file is inflated on the device.
 * ARX_E_TOO_LARGE: more than max_bytes; a line or record that a run does not hold with both buffers full, or more than 1024 runs (msg:
 * use a larger run_bytes); more than 2^32 - 1 records; buffers or a record table that the device does not hold.  ARX_E_IO as above, and a
 * tmp_dir in which no file can be made.  After any error neither outputs, .tmp files nor temporary files are left.
 * stats[24] (may be NULL): [0..19] as above ([10] counts the windows of all runs; without ARX_FQSORT_TIMED [16] is the device work of the
 * runs and [17] that of the merge, [14] and [15] are 0), [20] sorted runs written, [21] bytes of the temporary files, [22] microseconds
 * fetching and writing runs, [23] microseconds reading them back and uploading them. */
int arx_fastq_sort_ex(int32_t device, const char *r1_in, const char *r2_in, const char *r1_out, const char *r2_out, int32_t flags, int64_t max_bytes, int64_t run_bytes,
                      const char *tmp_dir, int64_t *stats, char *msg, int32_t msg_cap);
/* arx_selftest_fastq_sort's arguments and run_bytes (at least 128 and at least window_bytes, ARX_E_ARG below; window_bytes 0: min(run_bytes, 32 MiB)): the
 * orchestration of arx_fastq_sort_ex on two texts in host memory, the sorted runs held in host memory too (tests/test_fastq_sort_ext_gpu.py).
 * stats[24] as above.  On any error out1, out2, rec_off1 and rec_off2 are untouched. */
int arx_selftest_fastq_sort_ext(int32_t device, const uint8_t *t1, int64_t n1, const uint8_t *t2, int64_t n2, int64_t window_bytes, int64_t slab_bytes, int64_t run_bytes,
                                uint8_t *out1, uint8_t *out2, int64_t *out_len, int64_t *rec_off1, int64_t *rec_off2, int64_t *n_records, int64_t *stats);

/* ---- in front of the sort: the headers of a haplotagging, stLFR or TELLseq FASTQ pair rewritten on the GPU to the form the feeder's barcode
 * rule and the sort's key read, `@<id>/1\tBX:Z:<barcode>\tVX:i:<0|1>`.  The reference has this step half-written in
 * src/preprocess/standardize.go (format detection on the first 200 records, three converters, the rewrite of both headers); that file does
 * not compile (a dangling stdin.Write, convertFunc scoped inside its `if`, Valid concatenated as a string).  What is built is the intended
 * behaviour, with the repairs and deviations named where they apply.  The contract:
 *   record     exactly arx_fastq_sort's: lines exist only where they end in '\n'; R1 and R2 are walked in lockstep up to the shorter file's line
 *              count; while searching, a pair whose R1 line is non-empty and starts with '@' opens a record of four line pairs, any other pair
 *              is skipped; a record that the end of either file cuts off does not exist
 *   H          the R1 header without its '@', the line's own '\n' standing as closing white space.  White space (\s, \S below) is the feeder's
 *              set: ' ', \t, \n, \r, \v, \f, so that what this step calls a barcode is what the feeder will see; digits are 0-9.  R2's header
 *              plays no part and is dropped
 *   matchers   "the pattern matches at some position of H", each decidable by one forward scan from each candidate start:
 *                standard      BX:Z:(\S+)\s matches somewhere AND VX:i:([01])\s matches somewhere
 *                haplotagging  BX:Z:A\d\dC\d\dB\d\dD\d\d\s
 *                stLFR         #[0-9]+_[0-9]+_[0-9]+(/[12])?\s     (repair: standardize.go:22 has no (/[12])?, so it cannot match the #1_2_3/1
 *                                                                   that stLFR files carry)
 *                TELLseq       :[ATCGN]+\s                         (upper case only)
 *   detection  (findFastqFormat, standardize.go:102-127) records 0..199 in input order, fewer if the input has fewer; the first record that
 *              matches any pattern decides, the order of trial being standard, haplotagging, stLFR, TELLseq; no such record: unknown.  The
 *              reference applies the matchers to record.ReadInfo, which ParseHeader has stripped of its tags; the intended subject is H.
 *              Detection is a pass of its own over the head of the input (it looks at 4 MiB of each file first and at a whole parse
 *              window only where a record does not fit that, so its result does not depend on the window); files are opened again
 *              for the conversion
 *   conversion one format for the whole input.  barcode and v:
 *                haplotagging  the value of the leftmost BX:Z:(\S+)\s, the feeder's own rule; v = 1 iff it has no two adjacent '0' bytes
 *                              (repair: standardize.go:138 has the sense inverted)
 *                stLFR         the n_n_n of the leftmost stLFR match, without /1; v = 1 iff it does not start with "0_", contain "_0_" or end
 *                              in "_0" (stlfrInvalidRe: 00_1_2 and 10_2_3 are valid)
 *                TELLseq       the letters of the leftmost TELLseq match; v = 1 iff it holds no 'N' (repair: standardize.go:182 tests the wrong
 *                              variable)
 *              a record without a match has the empty barcode and v = 0 (the reference would print 1 for stLFR and TELLseq; the feeder
 *              reports such a record as not valid anyway)
 *   id         the first white-space-delimited token of H, leading white space skipped, one trailing /1 or /2 removed when the token ends in
 *              it; it may be empty; the token is otherwise kept whole, a #... or :ACGT part included
 *   output     per record, in input order: R1 gets '@' id "/1\tBX:Z:" barcode "\tVX:i:" v '\n' and lines 2-4 of the R1 record verbatim, R2 the
 *              same header with /2 and lines 2-4 of the R2 record verbatim; the header is 17 + |id| + |barcode| bytes.  (Deviations: the
 *              reference writes a blank line after the header, which would break the four-line record, and a bare '+'; lines 2-4 verbatim
 *              lose nothing.)  Skipped lines and the cut-off record are dropped
 * The property this exists for: where the id contains neither BX:Z: nor VX:i:, the host feeder reads from the output every record with
 * barcode and valid equal to the barcode and v above, info equal to the id (the feeder's own rule gives a record without a barcode no
 * info) and the bases and qualities of the input, and arx_fastq_sort of the output orders by that barcode.
 * format: ARX_FQSTD_AUTO detects first; 1..3 force a format and skip detection; anything else is ARX_E_ARG.  AUTO that finds standard
 * returns ARX_OK and writes nothing -- no output file and no .tmp is created, stats[6] says so, the caller uses its inputs; AUTO that
 * finds unknown is ARX_E_ARG (msg: no record of the first 200 names a format, pass one).  ARX_FQSTD_DETECT: only the detection runs, the
 * output paths may be NULL, and unknown is a result (ARX_OK, stats[6] = 5).  A forced format on an input of zero records gives two empty outputs.
 * Inputs may be plain text, gzip or BGZF, each file judged by itself; a BGZF file is inflated on the device, and with ARX_FQSTD_GUNZIP_DEVICE
 * a gzip file is inflated on the device too (in chunks: csrc/dev_gunzip.h), the detection's reads included.  Outputs are plain text, or with
 * ARX_FQSTD_BGZF BGZF files (blocks cut every 65280 bytes, the 28-byte EOF block last); they are written as <path>.tmp and renamed at the end:
 * a failing call leaves nothing behind.  The call streams: device memory holds the parse windows (32 MiB per file, twice), their carry and
 * the output slabs (64 MiB per file, twice), never a file; there is no size limit and no max_bytes (csrc/hip_fqstd.h has the accounting).
 * ARX_E_ARG: null paths without DETECT, unknown flag bits, a format outside 0..3, an output path that is an input or equals the other output;
 * ARX_E_IO: a file cannot be read or written, or a block does not inflate (nothing is produced); ARX_E_TOO_LARGE: a line or record that a
 * window does not hold; ARX_E_DEVICE: no GPU, or a HIP error -- there is no CPU fallback.
 * stats[20] (may be NULL): [0] records written, [1] [2] inflated bytes read from R1, R2 (the call stops reading where the input ends: a file
 * that goes on behind the other's last line is not read to its end), [3] [4] bytes written to R1, R2 as inflated text, [5] lines skipped,
 * [6] the format used or found, [7] the record that decided the detection (-1: forced, or none), [8] records with a barcode, [9] records
 * written with VX:i:1, [10] longest barcode, [11] parse windows, [12] output slabs, then microseconds: [13] waiting for the readers,
 * [14] upload and inflate, [15] parse, [16] fields and sizes (TIMED only, otherwise under [17]), [17] compose, [18] compress and write of BGZF
 * blocks, [19] fetch and write of plain text, last blocks, rename.  arx_fastq_prepare below is this step fused into the sort: one call, no
 * files between the two.  Not built: other header formats. */
enum { ARX_FQSTD_AUTO = 0, ARX_FQSTD_HAPLOTAGGING = 1, ARX_FQSTD_STLFR = 2, ARX_FQSTD_TELLSEQ = 3, ARX_FQSTD_STANDARD = 4, ARX_FQSTD_UNKNOWN = 5 }; /* 4, 5: results only */
enum { ARX_FQSTD_BGZF = 1, ARX_FQSTD_DETECT = 2, ARX_FQSTD_GUNZIP_DEVICE = 8, ARX_FQSTD_TIMED = 0x100 };
int arx_fastq_standardize(int32_t device, const char *r1_in, const char *r2_in, const char *r1_out, const char *r2_out, int32_t format, int32_t flags, int64_t *stats,
                          char *msg, int32_t msg_cap);
/* self-test of the same orchestration, detection pass included, on two texts in host memory (tests/test_fastq_standardize_gpu.py).
 * window_bytes and slab_bytes as in arx_selftest_fastq_sort (0: the defaults; a window of at least 128 and at most 2^29 bytes, ARX_E_ARG
 * outside).  out1[cap1], out2[cap2] receive the rewritten texts, out_len[2] their lengths, rec_off1 / rec_off2[*n_records + 1] where the
 * records start in them (room for n1 / 5 + 2 entries always suffices); cap1 or cap2 too small is ARX_E_TOO_LARGE -- 2 n1 + 17 (n1 / 5 + 2)
 * and 2 n1 + n2 + 17 (n1 / 5 + 2) always suffice, because id and barcode may overlap in H.  AUTO that finds unknown is ARX_E_ARG with
 * stats[6] = 5.  On any error, and where AUTO finds standard (ARX_OK, stats[6] = 4), out1, out2, out_len, rec_off1, rec_off2 and n_records are
 * untouched. */
int arx_selftest_fastq_standardize(int32_t device, const uint8_t *t1, int64_t n1, const uint8_t *t2, int64_t n2, int32_t format, int64_t window_bytes, int64_t slab_bytes,
                                   uint8_t *out1, int64_t cap1, uint8_t *out2, int64_t cap2, int64_t *out_len, int64_t *rec_off1, int64_t *rec_off2, int64_t *n_records,
                                   int64_t *stats);

/* ---- the two steps in front of the feeder as one: a haplotagging, stLFR or TELLseq FASTQ pair standardized AND sorted by barcode on the GPU,
 * without the files that arx_fastq_standardize writes and arx_fastq_sort_ex reads back (the reference means them as one preparation too:
 * main.go:85, preprocess.go and standardize.go).  The rule: for every input and every run_bytes the two outputs inflate to exactly the
 * bytes that arx_fastq_sort_ex writes for the files that arx_fastq_standardize(format) writes for the input.  So
 *   record, id, barcode, v   arx_fastq_standardize's, word for word; skipped lines and the cut-off record are dropped
 *   output      per record '@' id "/1\tBX:Z:" barcode "\tVX:i:" v '\n' ("/2" in R2) and lines 2-4 verbatim, ordered by the sort key as
 *               unsigned bytes, a proper prefix first, equal keys in input order; it does not depend on run_bytes, on window or slab sizes
 *               or on how the readers cut the input
 *   sort key    what the feeder's rule reads from the composed R1 header, the value of its leftmost BX:Z:(\S+)\s.  Normally that is the
 *               barcode.  Where the id itself contains BX:Z: it is the id's bytes behind its leftmost BX:Z: followed by "/1" (the id is the
 *               one above, a trailing /1 or /2 removed; BX:Z: cannot straddle the id and "/1"; "/1" makes the value non-empty and the
 *               '\t' closes it) -- a key in two pieces, the second not in the input: `xBX:Z:ab ...`, `y BX:Z:ab/1` and `zBX:Z:ab/1` all
 *               sort under ab/1, in input order.  No BX:Z: in the id and an empty barcode: the empty key
 *   detection   arx_fastq_standardize's, a pass of its own over the head of the input.  AUTO that finds standard: the call is exactly
 *               arx_fastq_sort_ex on the inputs -- the sorted files are written, this is a sort and no no-op; stats[26] and [27] are 0
 *               then.  AUTO that finds unknown: ARX_E_ARG, nothing is written, stats[24] = 5.  A forced format on zero records gives two
 *               empty outputs
 * flags are arx_fastq_sort_ex's: ARX_FQSORT_BGZF, ARX_FQSORT_TIMED, ARX_FQSORT_GUNZIP_DEVICE (a gzip file is inflated on the device), and ARX_FQSORT_CHECK -- nothing is written, the output paths may be
 * NULL, no temporary file is made, only stats is filled, and stats[6] == stats[7] says that the standardized input would need no sort.
 * max_bytes, run_bytes and tmp_dir are arx_fastq_sort_ex's too, with two differences: the run buffers hold RAW text while the temporary
 * files hold standardized text (the disk needed is the output's size), and run_bytes == -1 is a TENTH of the free device memory less 1 GiB
 * (whole MiB, at least 32 MiB, at most 16 GiB), because a record takes 120 bytes here where the sort has 80 (csrc/dev_fqprep.h: 40 more for
 * id, barcode, key and header ends): a run is 2 run_bytes + 2.4 run_bytes at 100 bytes of text per record and file, and a tenth keeps
 * the runs a little under half of the free memory as the sort's eighth does.  Nobody has measured which run size is fastest.  With
 * run_bytes == 0 both raw texts and 120 bytes per record stay in device memory.
 * Refusals are the union of the two calls'.  ARX_E_ARG: null paths without CHECK, unknown flag bits, a format outside 0..3, an output that
 * is an input or equals the other output, run_bytes below 128 other than 0 and -1.  ARX_E_IO: a file cannot be read or written, a BGZF block
 * does not inflate, tmp_dir is unusable.  ARX_E_TOO_LARGE: more than max_bytes; a line or record that a window or a run does not hold; more
 * than 1024 runs; more than 2^32 - 1 records; more than the device memory -- msg names the remedy.  ARX_E_DEVICE: no GPU, or a HIP error;
 * there is no CPU fallback.  After any error no output, .tmp or temporary run file is left, and the inputs are untouched.
 * stats[28] (may be NULL): [0..23] as arx_fastq_sort_ex's -- [1] [2] the inflated bytes read from the raw inputs, [3] [4] the bytes written
 * as inflated text, [5] lines skipped, [6] [7] [8] runs, distinct keys and the longest key, all by the sort key above --, [24] the format
 * used or found, [25] the record that decided the detection (-1: forced, or none), [26] records with a barcode, [27] records written with
 * VX:i:1. */
int arx_fastq_prepare(int32_t device, const char *r1_in, const char *r2_in, const char *r1_out, const char *r2_out, int32_t format, int32_t flags, int64_t max_bytes,
                      int64_t run_bytes, const char *tmp_dir, int64_t *stats, char *msg, int32_t msg_cap);
/* self-test of the same orchestration, detection pass included, on two texts in host memory, the sorted runs held in host memory too
 * (tests/test_fastq_prepare_gpu.py).  window_bytes and slab_bytes as in arx_selftest_fastq_sort; run_bytes 0 or at least 128 and at least
 * window_bytes (ARX_E_ARG otherwise; window_bytes 0: min(run_bytes, 32 MiB)).  out1[cap1], out2[cap2], out_len, rec_off1, rec_off2 and
 * n_records as in arx_selftest_fastq_standardize, the caps included; stats[28] as above.  AUTO that finds unknown is ARX_E_ARG with
 * stats[24] = 5.  On any error every output argument is untouched. */
int arx_selftest_fastq_prepare(int32_t device, const uint8_t *t1, int64_t n1, const uint8_t *t2, int64_t n2, int32_t format, int64_t window_bytes, int64_t slab_bytes,
                               int64_t run_bytes, uint8_t *out1, int64_t cap1, uint8_t *out2, int64_t cap2, int64_t *out_len, int64_t *rec_off1, int64_t *rec_off2,
                               int64_t *n_records, int64_t *stats);

/* ---- between the path and the sink: the placed candidate of every read of a super-batch as BAM records -- the part of DumpToBams /
 * AppendBam (src/aligner/bamwriter.go:283-568, 635-658) that decides flags, position, MAPQ, mate fields, template length, CIGAR op codes,
 * strand of bases and qualities and the RG / AS / XM / AM / XT / BX / VX tags of the primary record (csrc/bam_records.h lists what is left
 * to the caller: split records and their tags).  sb: the super-batch the batch was created from; cand_off / cands: arx_batch_rfa_fetch;
 * alns / cigars: arx_batch_fetch; post: arx_batch_post_fetch's per-candidate records or NULL (no duplicate flags).  The view points
 * into the buffer and stays valid until the next build on it; hand it to arx_bam_write.  Host code only. */
typedef struct arx_recbuf arx_recbuf;
int arx_recbuf_create(arx_recbuf **out);
int arx_recbuf_build(arx_recbuf *rb, const arx_super_batch *sb, const int32_t *cand_off, const arx_cand *cands, const arx_aln *alns, const uint32_t *cigars,
                     const arx_cand_post *post, int32_t threads, arx_bam_batch *view);
/* The reference's position buckets (CreateBAMs, bamwriter.go:134-188): a contig longer than chunk gets ceil(len / chunk) files of its own,
 * "%06d-<name>_%010d_pos_bucketed.bam" (contig index, chunk start); shorter contigs are packed into the current file while the running
 * size + len <= chunk (a multi-chunk contig does not reset the running size); "ZZZ_unmapped_pos_bucketed.bam" comes last.  A mapped record
 * of contig rid at pos goes to file contig_file[rid] + pos / chunk, an unmapped one to *n_files - 1.  file_names: cap_files rows of
 * name_w bytes (NUL-terminated), may be NULL; ARX_E_ARG when the table needs more rows or a longer row. */
int arx_bucket_table(int32_t n_contigs, const char *const *names, const int32_t *lens, int64_t chunk, int32_t *contig_file /* n_contigs */,
                     int32_t *n_files, char *file_names, int32_t cap_files, int32_t name_w);
/* The whole record set of DoDumpToBam (bamwriter.go:278-566, 635-689): every read's primary record, then its split record (flag 0x100,
 * hard-clipped) when arx_split names one, with the full tag set RG XS XC AC AS XM AM XT SA BX VX DM in the reference's order, and the
 * order effects of AppendBam's in-place "unmapped" mutation (pos = -1, mapq = 0 on a record the score rule unmaps, seen by every record
 * written after it).  n_records = 2 * n_pairs + splits.  DM is written on primary records only (see csrc/bam_records.h).  post is
 * required; bucket[n_records] (pointer into the buffer, valid with the view): the position bucket of every record per arx_bucket_table. */
typedef struct {
	const arx_split *split;         /* arx_batch_post_fetch: n_reads */
	const int32_t *mm_ref, *mm_read;/* arx_batch_post_fetch: the mismatch lists */
	const arx_read_tags *tags;      /* arx_batch_tags_fetch: n_reads */
	int32_t n_contigs, pad;
	const char *const *contig_names;/* for SA:Z */
	const int32_t *contig_file;     /* arx_bucket_table */
	int64_t chunk;
	int32_t unmapped_file, pad2;
} arx_recbuf_full;
int arx_recbuf_build_full(arx_recbuf *rb, const arx_super_batch *sb, const int32_t *cand_off, const arx_cand *cands, const arx_aln *alns, const uint32_t *cigars,
                          const arx_cand_post *post, const arx_recbuf_full *full, int32_t threads, arx_bam_batch *view, const int32_t **bucket);
const char *arx_recbuf_error(arx_recbuf *rb);
void arx_recbuf_free(arx_recbuf *rb);

/* ---- arx_recbuf_build -> arx_bam_write's encoder on the device: the records phase of a batch.  Writes the BAM-encoded primary record of
 * every read (the record set and rules of arx_recbuf_build above: csrc/bam_records.h RecBuf::build, then BamSink::encode, csrc/bam_sink.h;
 * bamwriter.go:283-568, 635-658) as one byte stream in device memory -- byte for byte what arx_recbuf_build -> arx_bam_write would append to a
 * writer -- from what arx_batch_rfa left there; the rules are csrc/bam_rules.h's on both sides.  sb: the super-batch the batch was created from; its
 * qualities, names, read groups, barcodes and set table are uploaded by the call (2 * sb->n_pairs == n_reads, sb->lens the batch's lengths,
 * names of 1..254 bytes: ARX_E_ARG before anything is launched otherwise).  flags bit 0: set 0x400 from arx_batch_post's duplicate marks
 * (ARX_E_ARG if arx_batch_post has not run); 0 = arx_recbuf_build with post == NULL.  Needs arx_batch_rfa first (ARX_E_ARG).  A read without an
 * active candidate: ARX_E_ARG; a stream of 2^31 - 1 bytes or more: ARX_E_TOO_LARGE, split the batch.  The phase comes last (after arx_batch_post
 * and arx_batch_tags): calling it again rebuilds it in the same memory, and a later arx_batch_run / _rfa / _post / _tags / _reset* discards it.
 * The call returns with the batch's stream synchronised: the stream of records is complete. */
int arx_batch_records(arx_ctx *ctx, arx_batch *b, const arx_super_batch *sb, int32_t flags, int64_t *n_records, int64_t *n_bytes);
/* stream[n_bytes]: the record stream as one block (hand it to arx_bam_write_encoded); rec_off[n_records + 1] (may be NULL): where each record starts */
int arx_batch_records_fetch(arx_ctx *ctx, arx_batch *b, uint8_t *stream /* n_bytes */, int64_t *rec_off /* n_records + 1, may be NULL */);
/* the stream in device memory (for arx_bam_write_encoded_device), valid until the phase is left -- the same contract and ordering rule as
 * arx_batch_device_view: the call waits for the batch's stream */
int arx_batch_records_view(arx_ctx *ctx, arx_batch *b, const uint8_t **d_stream, int64_t *n_bytes, int64_t *n_records);

/* ---- the reference's record set on the device: what arx_recbuf_build_full -> arx_bam_write would append (DoDumpToBam, bamwriter.go:278-566,
 * 635-689: primary and split records, the tags RG XS XC AC AS XM AM XT SA BX VX DM), byte for byte, and the same records a second time grouped
 * by position bucket (AppendBams writes every record to bc_sorted_bam.bam and to its bucket, :279-281; the files of CreateBAMs, :134-188),
 * built from what arx_batch_post and arx_batch_tags left in device memory.  The layout is arx_bucket_table's: n_files = unmapped_file + 1. */
typedef struct {
	const int32_t *contig_file;     /* arx_bucket_table: n_contigs */
	int32_t n_contigs;              /* must equal the context's (arx_contigs) */
	int32_t unmapped_file;          /* *n_files - 1 */
	int64_t chunk;
} arx_records_layout;
/* Needs arx_batch_rfa, arx_batch_post AND arx_batch_tags on the batch (ARX_E_ARG names the missing one).  The same phase as arx_batch_records
 * -- either call rebuilds it, a later arx_batch_run / _rfa / _post / _tags / _reset* discards it -- with the same checks of the super-batch.
 * n_records = n_reads + splits.  ARX_E_ARG also: a layout that is not the index's (n_contigs, a file outside [0, unmapped_file), a record whose
 * bucket lies outside the table), more than 4096 files (the grouping's table holds n_files entries per 256 records), an arx_split that names
 * a candidate of another read or one without an alignment (arx_recbuf_build_full's text).  ARX_E_TOO_LARGE: a stream of 2^31 - 1 bytes or
 * more, or a grouping table (n_files * ceil(n_records / 256) entries) above 2^26: split the batch or use a larger chunk.  Returns with both streams complete. */
int arx_batch_records_full(arx_ctx *ctx, arx_batch *b, const arx_super_batch *sb, const arx_records_layout *lay, int64_t *n_records, int64_t *n_bytes);
/* After arx_batch_records_full only (ARX_E_ARG when arx_batch_records ran last); any argument may be NULL.  bucket[n_records]: the bucket of
 * every record; grouped[n_bytes]: the records ordered by bucket, within a bucket in stream order (the stable order by bucket);
 * bucket_byte_off / bucket_rec_off[n_files + 1]: where bucket f's bytes / records start in it.  arx_batch_records_fetch / _view serve the
 * ungrouped stream of whichever of the two calls ran last. */
int arx_batch_records_buckets_fetch(arx_ctx *ctx, arx_batch *b, int32_t *bucket, uint8_t *grouped, int64_t *bucket_byte_off, int64_t *bucket_rec_off);
/* the grouped stream where it lies (bucket f: arx_bam_write_encoded_device(w, *d_grouped + bucket_byte_off[f], bytes, records)), the offsets
 * on the host; the contract of arx_batch_records_view */
int arx_batch_records_buckets_view(arx_ctx *ctx, arx_batch *b, const uint8_t **d_grouped, int64_t *bucket_byte_off, int64_t *bucket_rec_off);

/* ---- several GPUs behind one handle (arx_open(prefix, n_devices, ...)): one index replica per device, a super-batch of whole
 * barcodes cut by pair count (greedy longest-processing-time), every device's share on a host thread of its own, the result slabs
 * renumbered into the order of the read set -- byte for byte what ONE batch over everything returns.  devices: HIP device indices or NULL
 * for 0 .. n_devices - 1.  The result arrays are host memory owned by the handle, valid until the next call on it; device_of_barcode says
 * where each barcode ran.  (csrc/arx_multi.cpp: host code on the single-device entry points above; the reads reach every GPU from host
 * memory, so nothing travels between GPUs here -- arachne_amd/shard.py is the RCCL form for reads that arrive on one GPU.) */
typedef struct arx_multi arx_multi;
typedef struct {
	int64_t n_reads, n_regs, n_cigar, n_cands;
	const int32_t *reg_off; const arx_reg *regs; const arx_aln *alns; const uint32_t *cigars;
	const int32_t *cand_off; const arx_cand *cands;
	const int32_t *device_of_barcode; /* n_barcodes: index into the handle's devices */
} arx_multi_result;
int arx_multi_open(const char *prefix, int32_t n_devices, const int32_t *devices, arx_multi **out, char *msg, int32_t msg_cap);
int arx_multi_contigs(arx_multi *m, int32_t *n, const char *const **names, const int64_t **offsets, const int32_t **lens, const int32_t **is_alt, int64_t *l_pac);
int arx_multi_run(arx_multi *m, int32_t n_reads, const uint8_t *bases, const int32_t *lens, int32_t n_barcodes, const int64_t *bc_pair_off, const uint8_t *do_rfa,
                  double penalty, const int64_t *cen_start, const int64_t *cen_end, arx_multi_result *out);
const char *arx_multi_error(arx_multi *m);
void arx_multi_close(arx_multi *m);

/* intermediate results for parity tests (device -> host copies of stage outputs) */
#define ARX_CAP_INTV 256
int arx_batch_debug_intv(arx_ctx *ctx, arx_batch *b, int32_t *n_intv, uint64_t *intv4 /* n_reads*ARX_CAP_INTV*4 */);
/* Census of the backward sweeps of the SMEM passes (tests: which kernel took which task).  enable = 1 / 0 switches it on / off for the batch's
 * following arx_batch_run calls and clears the sums, enable < 0 leaves both alone; census8 (may be null) receives the sums as they were before
 * that: [0] backward launches, [1..4] tasks in the 16 / 21 / 32 / 64-lane bins of the row-parallel kernel, [5] tasks it (or the pipelined
 * one-lane kernel) flagged for the whole-wavefront kernel, [6] tasks left to text mode's tail, [7] length of the hand-off lists the
 * whole-wavefront kernel was given.  Off (the default) nothing is counted and nothing is copied; on, each backward launch costs one more
 * device-to-host copy of its bookkeeping.  The host test double keeps no census and reports zeros. */
int arx_batch_debug_seed_census(arx_ctx *ctx, arx_batch *b, int32_t enable, int64_t *census8);
/* Census of the heavy-item lists (tests: which reads and pairs the wavefront-per-item kernels took); enable and census8 as above.
 * [0] chaining stages run, [1] reads listed for the chaining kernel's launch of up to 256 seed occurrences, [2] for its launch above that,
 * [3] reads listed for the de-duplication kernel, [4] pairs listed for the rescue replay, [5..7] those pairs by the LDS class of their two
 * list capacities together (up to 170 / 340 / 680 records) when the replay is launched per class (ARX_RESCUE_LDS_CLASSES=1), otherwise all
 * in [7].  Off (the default) nothing is counted and nothing is copied; on, each of the three stages costs device-to-host copies of its
 * list.  The host test double keeps no census and reports zeros. */
int arx_batch_debug_heavy_census(arx_ctx *ctx, arx_batch *b, int32_t enable, int64_t *census8);
int arx_batch_debug_chains(arx_ctx *ctx, arx_batch *b, int32_t *occ_off /* n_reads+1 */, int32_t *n_chain, arx_chain *chains, arx_seed *seeds /* counts[3] each */);
/* The split chaining's classification of the last chaining stage (tests): who[r] = 0 the light reads' launch, 1 the heavy launches, 2 the
 * listed reads' launch; heavy_list (n_reads entries) with n[0] of them filled; mid_list (n_reads / 4 + 64 entries) with min(n[1], n[2]) of
 * them filled, n[1] = reads that asked for a place, n[2] = the list's capacity (0: no such list).  ARX_E_ARG where the stage ran unsplit. */
int arx_batch_debug_chain_class(arx_ctx *ctx, arx_batch *b, uint8_t *who /* n_reads */, int32_t *heavy_list, int32_t *mid_list, int32_t *n /* 3 */);
/* 1: a batch handle created with ARX_AUX_STREAM unset runs its narrow launches on side streams -- GPU_MAX_HW_QUEUES was at least
 * ARX_HW_QUEUES (8) when the library was loaded, or the library raised it before the process opened the GPU; 0: it runs on one stream,
 * because the process had the GPU open with fewer queues.  libarachne_amd.so only. */
int32_t arx_side_streams_default(void);
int arx_batch_debug_core(arx_ctx *ctx, arx_batch *b, int32_t *n_core, arx_reg *regs /* counts[3] */);

/* self-test of a device routine that has no host twin (tests): klib's introsort as a wavefront reproduces it (csrc/dev_regs_wave.h:
 * w_introsort -- its order of equal keys is part of every result that passes mem_sort_dedup_patch or mem_chain_flt, ksort.h:176-226)
 * against the one-thread ks_introsort, on n_cases random index arrays of 2..832 entries whose keys come from small ranges, so that ties
 * abound.  *n_bad = arrays on which the two differ. */
int arx_selftest_wave_sort(int32_t device, int32_t n_cases, int64_t seed, int64_t *n_bad);

/* self-test of the device sink's kernels on arbitrary bytes, no index needed (tests/test_bgzf_device_gpu.py): src[0..n) is cut every 65280
 * bytes as the sink cuts its stream and goes through the kernels of arx_bam_open_device; out[0..*out_len) receives the framed BGZF blocks
 * in order, without the EOF block (cap: bytes of out; n + 31 * blocks always suffice; ARX_E_ARG if it is too small).  stats[4] (may be
 * NULL): blocks, and how many of them went out stored, with the fixed code, with a dynamic code.  n = 0: no block, *out_len = 0. */
int arx_selftest_bgzf(int32_t device, const uint8_t *src, int64_t n, uint8_t *out, int64_t cap, int64_t *out_len, int64_t *stats);

/* self-test of the device inflate's kernel on arbitrary BGZF blocks, no index needed (tests/test_inflate_gpu.py): src[0..n) is a chain of
 * whole BGZF blocks; its headers are walked on the host with the function the device feeder's reader thread uses, every block goes through
 * the kernel of arx_feeder_open_device_ex (csrc/dev_inflate.h, hip_inflate.h).  out receives the inflated bytes of all blocks in order, a
 * block's at the sum of ISIZE in front of it (cap: bytes of out; that sum must fit, else ARX_E_ARG); a block that is not ARX_INFLATE_OK
 * leaves its bytes of out as they were.  status[b] (status_cap entries; more blocks: ARX_E_ARG) is block b's status, one of ARX_INFLATE_*;
 * *out_len counts the bytes up to the first bad block.  Returns ARX_OK when every block is ARX_INFLATE_OK, ARX_E_IO when one is not, and
 * ARX_E_ARG for a chain whose headers do not tile src (no gzip magic, no BC subfield, a BSIZE that runs past n).  stats[4] (may be NULL):
 * blocks, compressed bytes (n), inflated bytes (the sum of ISIZE), DEFLATE blocks read.  n = 0: no block, *out_len = 0. */
enum { ARX_INFLATE_OK = 0, ARX_INFLATE_BAD_HEADER, ARX_INFLATE_BAD_BTYPE, ARX_INFLATE_BAD_STORED_LEN, ARX_INFLATE_BAD_CODE_LENGTHS, ARX_INFLATE_BAD_SYMBOL,
       ARX_INFLATE_BAD_DISTANCE, ARX_INFLATE_TRUNCATED, ARX_INFLATE_SIZE_MISMATCH, ARX_INFLATE_CRC_MISMATCH };
int arx_selftest_inflate(int32_t device, const uint8_t *src, int64_t n, uint8_t *out, int64_t cap, int64_t *out_len, int32_t *status, int32_t status_cap,
                         int64_t *stats);

/* self-test of the chunked inflate of a plain gzip file (one DEFLATE stream per member, no BGZF framing) on bytes in host memory, no index and
 * no file needed (tests/test_gunzip_gpu.py; csrc/dev_gunzip.h, hip_gunzip.h, gunzip_host.h).  src[0..n) is the file.  Its members' bodies are cut
 * into chunks of chunk_bytes compressed bytes, slab_bytes of them to a launch; every chunk looks for a DEFLATE block start in its range and
 * decodes from there into 16-bit symbols on the device, the windows are handed down the chain of chunks and the back-references into
 * unknown history replaced.  The framing (member headers, trailers, CRC-32 and length, the next member) is the calling thread's.  Whatever the
 * device does not take hands the rest of the file to zlib on the host.  The yardstick is zlib's gzread: out[0..*out_len) receives the bytes
 * gzread reads from the same file (members one after the other; bytes behind the last member that do not start a gzip header are ignored; a
 * file without the gzip magic comes back as it is), and where gzread reports an error the entry returns ARX_E_IO and *out_len is 0.
 * chunk_bytes: 0 for the default (32 KiB: the fastest of 32 / 64 / 128 KiB in profiles/device_gunzip), else at least 64.  slab_bytes: 0 for the default (8 MiB; not measured), else at
 * least 2 * chunk_bytes, at most 128 MiB and at most 16384 * chunk_bytes (a 32 KiB window is kept per chunk of a launch).  expand: 16-bit staging symbols per compressed byte, 0 for the default (8; not measured), at
 * most 1032, and slab_bytes * expand at most 2^30; a chunk that inflates to more is an overflow and goes to the host.
 * stats[ARX_GUNZIP_N_STATS] (may be NULL): [0] members, [1] compressed bytes consumed, [2] inflated bytes, [3] launches, [4] chunks, [5] chunks
 * with a candidate block start, [6] chunks accepted, [7] candidates refuted, [8] DEFLATE blocks decoded on the device, [9] marker symbols
 * replaced, [10] bytes inflated by the host, [11] why the host took over (ARX_GUNZIP_FB_*: the first reason; 0: it did not), [12] bytes
 * ignored behind the last member, [13..15] microseconds of the launches' phases: find, decode, windows and resolve together.
 * Returns ARX_OK, ARX_E_IO as said, ARX_E_ARG for sizes outside their bounds or a cap below the inflated size, ARX_E_TOO_LARGE where host or
 * device memory does not hold a launch's buffers, ARX_E_DEVICE without a GPU. */
enum { ARX_GUNZIP_FB_NONE = 0, ARX_GUNZIP_FB_REFUTED, ARX_GUNZIP_FB_OVERFLOW, ARX_GUNZIP_FB_STATUS, ARX_GUNZIP_FB_CHECK, ARX_GUNZIP_FB_NO_BLOCK, ARX_GUNZIP_FB_CUT_SHORT };
enum { ARX_GUNZIP_N_STATS = 16 };
int arx_selftest_gunzip(int32_t device, const uint8_t *src, int64_t n, int64_t chunk_bytes, int64_t slab_bytes, int32_t expand, uint8_t *out, int64_t cap, int64_t *out_len,
                        int64_t *stats);

/* What the gzip inputs of the file-pair calls did on the device (ARX_FQSORT_GUNZIP_DEVICE, ARX_FQSTD_GUNZIP_DEVICE), summed over the process
 * since it started or since the last call with reset != 0; a file is booked when its reading ends, by the end of the file, an error or the end
 * of a detection.  counters[ARX_GUNZIP_N_COUNTERS]: [0] gzip files the device was given, [1] launches, [2] chunks accepted, [3] bytes of text
 * delivered, [4] of them inflated by the host's zlib, [5] unused, [6..11] files in which the host took over, by the first reason
 * ARX_GUNZIP_FB_REFUTED .. ARX_GUNZIP_FB_CUT_SHORT.  No device is touched. */
enum { ARX_GUNZIP_N_COUNTERS = 12 };
int arx_fastq_gunzip_counters(int64_t *counters, int32_t reset);

/* self-test of the decimal text the records phase writes on the device (csrc/dev_records_full.h), one input per lane: kind 0: "%d" of a[i]
 * (b is not read); kind 1: "%.6f" of (double)a[i] / (double)b[i], b[i] > 0 (else ARX_E_ARG).  out: n rows of 32 bytes, len[n]: the bytes
 * of each text.  There so that the GPU suite can hold the formatters to the host's on inputs the path does not produce at test size. */
int arx_selftest_rec_text(int32_t device, int32_t n, const int32_t *a, const int32_t *b, int32_t kind, uint8_t *out /* 32 * n */, int32_t *len /* n */);

/* self-test of the workgroup primitives the placement kernel is written in (csrc/hip_block.h: exclusive_scan, sort_kv, argmax), one case per
 * workgroup, started through k_block_items like the kernel itself.  klass 0: BLOCK_LANES lanes and SORT_LDS sort entries of LDS, 1: SMALL_LANES
 * and SMALL_SORT.  Case c reads keys / vals at [in_off[c], in_off[c] + n[c]) and writes out_keys / out_vals from out_off[c] on:
 *   ARX_BLOCK_OP_SCAN    out_vals[0 .. n] = sums of vals in front of each index (n + 1 values), out_vals[n + 1 .. n + 4] = the value the call
 *                        returned in lanes 0, 63, 64 and the last one;
 *   ARX_BLOCK_OP_SORT    the n pairs (n a power of two) ascending by (key, (uint32)val); above the class's sort entries the sort runs in HBM;
 *   ARX_BLOCK_OP_ARGMAX  out_keys / out_vals[0 .. 3] = the largest key (0: none) and its smallest index (0x7fffffff: none) as those four lanes got them.
 * Everything else of out_keys / out_vals (n_out entries each) comes back as the caller filled it.  Offsets outside the arrays: ARX_E_ARG. */
enum { ARX_BLOCK_OP_SCAN = 0, ARX_BLOCK_OP_SORT = 1, ARX_BLOCK_OP_ARGMAX = 2 };
int arx_selftest_block_shape(int32_t klass, int32_t *lanes, int32_t *sort_entries); /* the two numbers of a class as this library was built (no device needed) */
int arx_selftest_block(int32_t device, int32_t klass, int32_t n_cases, const int32_t *op, const int32_t *n, const int64_t *in_off, const int64_t *out_off,
                       const uint64_t *keys, const int32_t *vals, int64_t n_in, uint64_t *out_keys, int32_t *out_vals, int64_t n_out);

/* self-test of the placement stage (what arx_batch_rfa runs: candidates per read, per-barcode joint placement, MAPQ with its host patch) on
 * alignments the caller made up, in the int64 row layout of the CPU restatement (oracle/arx_oracle.h: 20 columns per region, 12 per
 * alignment, CIGAR words at column 8's offset; n_cig words in all).  ann_off[n_seqs], l_pac: the only things read of an index.  rfa_small and
 * mapq_guard (< 0: the default) stand for ARX_RFA_SMALL and ARX_MAPQ_GUARD, which this entry does not read.  cands: cand_cap records of 96
 * bytes (api.py CAND_DTYPE), cand_cap = one per region plus one per read without any (else ARX_E_ARG); cand_off[n_reads + 1]; bc_out:
 * n_barcodes x (double dna_len, int32 n_mol, int32 pad -- diagnostics: the fastScore sweeps the barcode ran); cls[n_barcodes]: 1 where the barcode was given to the small workgroup class;
 * *n_host_mapq: reads whose MAPQ the host re-evaluated.  Row values that a kernel would index with are checked first (ARX_E_ARG). */
int arx_selftest_rfa(int32_t device, int32_t n_reads, const int64_t *reg_off, const int64_t *regs, const int64_t *alns, const uint32_t *cigars, int64_t n_cig,
                     const int32_t *lens, int32_t n_barcodes, const int64_t *bc_pair_off, const uint8_t *do_rfa, int32_t penalty, int64_t l_pac,
                     const int64_t *ann_off, int32_t n_seqs, const int64_t *cen_start, const int64_t *cen_end, int32_t rfa_small, double mapq_guard,
                     int32_t *cand_off, void *cands, int64_t cand_cap, void *bc_out, uint8_t *cls, int64_t *n_host_mapq);

/* self-test of the bins of the row-parallel backward sweeps, which the forward seeding kernels fill as they hand out pool slices
 * (csrc/hip_fm_coop.h grant step, csrc/dev_fm.h seed_bwd_class): the seeding stage of the given reads (bases: codes 0..4 back to back, any
 * n_reads >= 1) runs on a runtime of its own with ctx's index and the ARX_* switches as they are at the call, and what device memory holds
 * after every forward launch comes home.  Launch i (first pass and re-seeding pass of each group of reads, in that order): rec[8 i ..] =
 * first task, tasks, the four bins' counters, the batch's error word so far, 0; task_n: the list length of each of the launch's tasks;
 * bin_ids: the four bins' task ids, bin after bin.  task_n and bin_ids are appended launch after launch.  *n_launches: launches recorded.
 * ARX_E_TOO_LARGE: a cap is too small; an error word that is not 0 is no failure of this entry. */
int arx_selftest_seed_bins(arx_ctx *ctx, const uint8_t *bases, const int32_t *lens, int32_t n_reads, int32_t *n_launches, int32_t *rec, int32_t rec_cap,
                           int32_t *task_n, int64_t task_cap, int32_t *bin_ids, int64_t bin_cap);

/* self-test of the CIGAR stage (stage 6: what arx_batch_run does last -- classification by the first band, the 16-lane kernel per band class with
 * its band retries, the launch that takes what the class kernels hand on, the one-thread path for long regions, the retry of the whole stage with
 * wider CIGAR slots, and the compaction behind it) on regions the caller made up.  The stage runs on a runtime of its own with ctx's index and the
 * ARX_* switches as they are at the call.  Read r has cap[r] region slots of which the first n_regs[r] are used (0 <= n_regs[r] <= cap[r]; cap 0
 * is allowed); regs holds one row per SLOT (sum of cap rows, slot after slot; rows of unused slots are not read) in the int64 layout of the CPU
 * restatement (oracle/arx_oracle.h: 20 columns).  Checked before anything is uploaded (ARX_E_ARG): 0 <= lens <= 255; per used row 0 <= qb < qe
 * <= len, 0 <= rb < re <= 2 l_pac with both ends on one strand, re - rb <= 4096, w >= 0, |truesc| and the copied fields below 2^24, at most 2^20
 * slots -- a region bwa_gen_cigar2 rejects (bwa.c:126-134) is refused, the reference reads a score it never set there.
 * Out: reg_off[n_reads + 1], alns (aln_cap records of arx_aln, one per used region in read order) and cigars (cig_cap words, *n_cig used) as
 * arx_batch_fetch hands them out; *err: the batch's error word (ERR_POOL_OVERFLOW = 4: a long region's matrix did not fit, its record has rid -1
 * and no CIGAR; ERR_CIGAR_OVERFLOW = 8: 1024 words per region did not suffice, nothing is handed out).  ARX_E_TOO_LARGE: a cap is too small.
 * census (may be NULL: nothing is copied; else census_cap values): [0] the final CIGAR slot width  [1] passes of the slot loop; of the last pass
 * [2] regions queued for the 16-lane kernel  [3] regions too long for it  [4..8] the queued ones per band class  [9] regions the class kernels
 * handed on (-1: this runtime keeps no such list -- ARX_SW_SIMPLE, the host test double)  [10] n = rows that follow  [11] bit i: value [i] is
 * known to this runtime; then n rows (index of the region among the used ones, band class, 64-byte units of traceback matrix it was given).
 * grid_cap > 0: at most that many workgroups per class launch and two for the launch behind them (the grid-stride loops then take many regions
 * per group, one after the other through the same LDS rows); 0: the launch shapes of arx_batch_run. */
int arx_selftest_reg2aln(arx_ctx *ctx, const uint8_t *bases, const int32_t *lens, int32_t n_reads, const int32_t *cap, const int32_t *n_regs, const int64_t *regs,
                         int32_t *reg_off, void *alns, int64_t aln_cap, uint32_t *cigars, int64_t cig_cap, int64_t *n_cig, uint32_t *err, int64_t *census,
                         int64_t census_cap, int32_t grid_cap);

/* self-test of the passes between placement and the BAM records (what arx_batch_post runs: GetAlignments' CIGAR walk with the mismatch lists and
 * `matches`, markDuplicates, CheckSplitReads) on candidates the caller made up, in the int64 row layouts of the CPU restatement (oracle/arx_oracle.h;
 * ora_post takes the same arrays): cands holds cand_off[n_reads] rows of 20 columns (reg read pos aend reversed rid score ... lap2 active ...), read
 * after read; regs (20 columns, only qb / qe are read) and alns (12 columns, only NM / n_cigar / cigar_off are read) hold n_regs rows, a candidate's
 * column `reg` names its row (-1: the placeholder of a read without hits); cigars: n_cig words; bases: the reads back to back (codes 0..4).  The
 * stage runs on a runtime of its own with ctx's index (pac, contig offsets and lengths) and the ARX_* switches as they are at the call.
 * Checked before anything is uploaded (ARX_E_ARG): n_reads even, 0 <= lens <= 255, every read has a candidate and its rows carry its id, reg inside
 * [-1, n_regs), rid inside [0, n_seqs) (-1 allowed for a placeholder), -1 <= pos, 0 <= aend, both below 2^31, pos <= aend <= pos + 2^18, reversed
 * and active 0 or 1, |score|, |lap2|, |qb|, |qe|, |NM| at most 2^24, at most 64 CIGAR words per alignment inside [0, n_cig), each of length <= 4096,
 * barcodes that tile the pairs, both centromere arrays (n_seqs values each) or neither.
 * Out: post (cand_off[n_reads] records of 24 bytes: qb qe matches n_mm mm_off duplicate), split (n_reads records of 32 bytes: split mapq is_proper
 * n_split_cand order_pinned second_best2 score2 pad), mm_ref / mm_read (*n_mm locations; ARX_E_TOO_LARGE with *n_mm set when mm_cap is smaller).
 * table (may be NULL: nothing of it is copied): the duplicate table as the launches leave it in device memory (*n_table slots of read ids, -1: free;
 * ARX_E_TOO_LARGE when table_cap is smaller), and home[n_reads]: the slot each read's key hashes to, written by the table's own hash function.
 * grid_cap > 0: every thread-per-item launch on at most that many workgroups of 64 lanes, which stride through the items; 0: the launch shapes of
 * arx_batch_post.  order: the item order of the host test double's launches (0 ascending, 1 descending, 2 a stride permutation); the library
 * ignores it -- the order in which a GPU's lanes arrive is nobody's to choose. */
int arx_selftest_post(arx_ctx *ctx, int32_t n_reads, const int64_t *cand_off, const int64_t *cands, int64_t n_regs, const int64_t *regs, const int64_t *alns,
                      const uint32_t *cigars, int64_t n_cig, const uint8_t *bases, const int32_t *lens, int32_t n_barcodes, const int64_t *bc_pair_off,
                      int32_t penalty, const int64_t *cen_start, const int64_t *cen_end, void *post, void *split, int32_t *mm_ref, int32_t *mm_read,
                      int64_t mm_cap, int64_t *n_mm, int32_t *table, int64_t table_cap, int32_t *n_table, int32_t *home, int32_t grid_cap, int32_t order);

/* self-test of the extension stage (what arx_batch_run runs between chaining and mate rescue: one state machine per chain, the rounds of
 * ext_step / run_extend, the gather in chain order, mem_sort_dedup_patch) on chains and seeds the caller made up, in the int64 row layouts of the CPU
 * restatement (oracle/arx_oracle.h; ora_chain2aln takes the same rows): chains holds sum(n_chain) rows of 8 columns (pos rid n seed_off w kept first
 * is_alt), read after read, seed_off counting within the read's seed rows; seeds holds sum(n_seed) rows of 4 columns (rbeg qbeg len score);
 * frac_rep_bits: one value per read (mem_chain gives every chain of a read the same); bases: the reads back to back (codes 0..4).  The stage runs on
 * a runtime of its own with ctx's index and the ARX_* switches as they are at the call.
 * Checked before anything is uploaded (ARX_E_ARG), what mem_chain2aln's assert(c->rid == rid) and its fetches accept: 1 <= lens <= 255; every seed of
 * a chain in one contig and strand, rid that contig; 0 <= qbeg, qbeg + len <= lens, len >= 1, score == len; the chains' seed rows follow each other
 * inside the read's; at most 2^22 chain and seed slots.  A chain may be empty (n == 0), a read may have no chain.
 * Out: ext_off[n_reads + 1] and ext_regs: the regions after the gather, before the de-duplication (rows of 20 columns as the restatement's, frac_rep as
 * its bits); core_off[n_reads + 1], core_regs, core_clean[n_reads]: the lists the stage leaves (reg_cap rows each; sum(n_seed) suffice, ARX_E_TOO_LARGE
 * below that); stats: [0] n_ext_tasks [1] ext_rounds [2] rounds of the loop [3] chains; rounds (rounds_cap rows of 9: round number, chains still
 * active after it, tasks queued per query-length class); done_round and chain_n_regs per chain; *err: the batch's error word.
 * grid_cap > 0: every launch of the stage on at most that many workgroups; 0: the launch shapes of arx_batch_run.  order: the item order of the host
 * test double's launches (0 ascending, 1 descending, 2 a stride permutation); the library ignores it. */
int arx_selftest_ext_stage(arx_ctx *ctx, const uint8_t *bases, const int32_t *lens, int32_t n_reads, const int32_t *n_chain, const int64_t *chains, const int32_t *n_seed,
                           const int64_t *seeds, const uint32_t *frac_rep_bits, int32_t *ext_off, int64_t *ext_regs, int32_t *core_off, int64_t *core_regs,
                           int64_t reg_cap, int32_t *core_clean, int64_t *stats, int32_t *rounds, int64_t rounds_cap, int32_t *done_round, int32_t *chain_n_regs,
                           uint32_t *err, int32_t grid_cap, int32_t order);

/* self-tests of the three DP kernel families on plain host arrays (csrc/arx_selftest.hip; tests/test_dp_kernels_gpu.py): each entry
 * uploads the tasks, launches the production code on them and returns one result row per task, in input order.  The reference text is
 * passed in bwa's .pac layout (pac: (l_pac + 3) / 4 bytes, 2 bits per base, first base in the top bits); coordinates are doubled, so a
 * position >= l_pac reads the reverse strand as the path does.  Input outside what the pipeline guarantees is refused with ARX_E_ARG before
 * anything is launched.
 *
 * arx_selftest_extend: ksw_extend2 (end bonus 5, z-drop 100) by HipRT::run_extend.  task8: n rows of (tpos, qoff, qlen, tlen, qdir, tdir,
 * w, h0); the query base j is bases[qoff + j * qdir], the target base i is at doubled coordinate tpos + i * tdir.  Contract: 1 <= qlen <= 255,
 * qdir, tdir = +1 / -1, the query inside bases[0, n_bases), tlen >= 0 with the whole target on one strand of [0, 2 * l_pac) (tlen == 0: the window
 * ends where the seed does, at a contig's edge; no target base is read and tpos may be any value), w >= 1,
 * 1 <= h0 <= 255.  mode 0: one launch per query-length class, 1: all classes in one launch, 2: round 2's kernel (per class), 3: the
 * one-thread form.  grid_cap > 0: at most that many workgroups per launch (the grid-stride loops then take several tasks per group).
 * res6: n rows of (score, qle, tle, gtle, gscore, max_off).
 *
 * arx_selftest_rescue_sw: the rescue Smith-Waterman of mem_matesw (ksw_align2 of the reverse-complemented mate against the window, bwamem_pair.c:
 * 150) by HipRT::run_sw_u8.  Mate k is mates[mate_off[k], + mate_len[k]) in forward orientation, its window [win2[2k], win2[2k + 1]).  Contract:
 * 1 <= mate_len <= max_len <= 255, 1 <= window length <= 800, the window on one strand of [0, 2 * l_pac).  max_len picks the kernel as a batch's
 * longest read does; filter = 1 runs the pre-filter in front; sw_simple = 1 the one-thread form.  res7: (score, te, qe, score2, te2, tb, qb);
 * a task the pre-filter drops gets (0, -1, -1, -1, -1, -1, -1).
 *
 * arx_selftest_gen_cigar: bwa_gen_cigar2 on regions already oriented (query and target as ksw_global2 reads them) by the 16-lane CIGAR kernel of
 * band class klass (0..4: <1,2> <2,4> <4,8> <8,16> <16,16> columns per lane), or 5 for the <1,16> kernel that takes the punted regions.  w: the
 * band bwa_gen_cigar2 is called with.  Contract: 1 <= qlen <= 256, 1 <= tlen <= 1024, w >= 0, 1 <= cap[k] <= cig_w.  out4: (score, n_cigar,
 * NM, punted); cigar: cig_w words per task.  punted = 1: the band needs a wider tiling than the kernel holds (nothing else is set); NM = -1 when
 * n_cigar > cap. */
int arx_selftest_extend(int32_t device, const uint8_t *pac, int64_t l_pac, const uint8_t *bases, int64_t n_bases, int32_t n, const int64_t *task8,
                        int32_t mode, int32_t grid_cap, int32_t *res6);
int arx_selftest_rescue_sw(int32_t device, const uint8_t *pac, int64_t l_pac, const uint8_t *mates, int64_t n_bases, int32_t n, const int32_t *mate_off,
                           const int32_t *mate_len, const int64_t *win2, int32_t max_len, int32_t filter, int32_t sw_simple, int32_t grid_cap, int32_t *res7);
int arx_selftest_gen_cigar(int32_t device, int32_t n, const uint8_t *q, const int32_t *q_off, const int32_t *qlen, const uint8_t *t, const int32_t *t_off,
                           const int32_t *tlen, const int32_t *w, const int32_t *cap, int32_t cig_w, int32_t klass, int32_t *out4, uint32_t *cigar);

/* per-kernel device time (HIP events on the launch stream), accumulated since the last reset */
int arx_kernel_times(arx_ctx *ctx, int32_t cap, char *names, int32_t name_w, double *ms, int64_t *calls, int64_t *items);
void arx_kernel_times_reset(arx_ctx *ctx, int32_t enable);

#ifdef __cplusplus
}
#endif
#endif

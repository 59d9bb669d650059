// switches.h -- every ARX_* environment switch of the library: its parse convention, its default and when it is read.  Host-only C++17 (the
// host test double includes it too); the only file of csrc/ and tests/hostsim/ that calls getenv.  DESIGN.md section 13 is the same list as a
// table (tests/test_switches.py holds the two together).
//
// A switch is one field of one of the structs below; its default member initialiser reads the environment, so a struct is a snapshot taken
// where it is constructed and nothing is cached per process: a caller (a test) may change the environment between two handles.
//   IndexSwitches        constructed in Context::open (arx_open)
//   IndexBuildSwitches   constructed per arx_index_build call (product_bwt_sa)
//   BatchSwitches        a member of HipRT: read when the batch handle, context or device feeder that owns the runtime is created, never again
//   PipelineSwitches     a member of Pipeline, which a batch handle creates beside its runtime: read then, never again.  (Pipeline's own, not
//                        something it asks its RT for: the runtime interface stays functions only, and a test double need not carry one)
//   FeederSwitches       a member of DeviceFeeder: read when the device feeder is created
// The host double's own switches (ARX_SIM_*, ARX_RESCUE_FAST, ARX_RESCUE_CHECK, ARX_RESCUE_STATS, ARX_BWD_STATS) are declared in
// tests/hostsim/sim.cpp through the same helpers.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <dirent.h>
#include <unistd.h>

namespace arx {

// ---- parse helpers: one per convention.  Every switch keeps the convention it was introduced with; which one is part of its row.
inline bool sw_present(const char *name) { return getenv(name) != nullptr; }                                             // set to anything, "0" and "" included: on
inline bool sw_on_unless_zero(const char *name) { const char *e = getenv(name); return !(e && atoi(e) == 0); }           // unset: on; a value atoi reads as 0 (text included): off
inline bool sw_off_unless_nonzero(const char *name) { const char *e = getenv(name); return e && atoi(e) != 0; }          // unset: off; a value atoi reads as non-zero: on
inline int sw_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
inline uint64_t sw_u64(const char *name, uint64_t dflt) { const char *e = getenv(name); return e ? strtoull(e, nullptr, 10) : dflt; }
inline std::optional<int> sw_int_if_set(const char *name) { const char *e = getenv(name); return e ? std::optional<int>(atoi(e)) : std::nullopt; } // unset is a state of its own (the default is computed, or is a constant of another header)
inline std::optional<long> sw_long_if_set(const char *name) { const char *e = getenv(name); return e ? std::optional<long>(atol(e)) : std::nullopt; }
inline std::optional<double> sw_double_if_set(const char *name) { const char *e = getenv(name); return e ? std::optional<double>(atof(e)) : std::nullopt; }

// ---- index switches: what arx_open builds beside the index files (api_impl.h Context::open)
struct IndexSwitches {
	std::optional<int> kmer_k = sw_int_if_set("ARX_KMER_K"); // K of the third seeding pass's k-mer table; unset: computed from the genome size; 0: no table
	bool kmer_fwd = sw_on_unless_zero("ARX_KMER_FWD");       // 0: no per-depth levels for the forward extensions of the SMEM pass (the forward kernels walk base by base)
	bool text_index = sw_on_unless_zero("ARX_TEXT_INDEX");   // 0: never the whole suffix array and its inverse (text mode off, locate walks a sample)
	int sa_dense = sw_int("ARX_SA_DENSE", 4);                // rows per suffix-array sample without the whole array, a power of two; at least the file's interval switches it off.  Every 4th row since round 3 (12 GB at GRCh38 size; locate 4.9 -> 2.5 ms per step, arx_open +1.7 s); 8 in round 2
};

// ---- index-build switches (arx_index.hip product_bwt_sa, hip_index_build.h build_bwt_sa_device)
struct IndexBuildSwitches {
	bool host = sw_off_unless_nonzero("ARX_INDEX_HOST");              // 1: the host's induced sorting even when a device is visible (2 * l_pac < 2^31)
	int device = sw_int("ARX_INDEX_DEVICE", -1);                      // the device the suffix sort runs on; -1: the current one
	bool verbose = sw_present("ARX_INDEX_VERBOSE");                   // diagnostics: the build's steps on stderr
	bool verify = sw_on_unless_zero("ARX_INDEX_VERIFY");              // 0: skip the check of the finished order
	uint64_t chunk = sw_u64("ARX_INDEX_CHUNK", (uint64_t)512 << 20);  // suffixes per sorted chunk (tests shrink it so that small genomes take several); below 1: 1
	uint64_t slice = sw_u64("ARX_INDEX_SLICE", (uint64_t)256 << 20);  // rows per emitted slice; below 1: 1
};

// ---- the HIP runtime's hardware queues.  The runtime gives a process GPU_MAX_HW_QUEUES of them (4 unless set) and streams beyond that number
// share one, where the packets of two streams run in order: a tail on one batch's side stream then sits in front of another batch's main
// stream, and the side streams cost 10 % of the throughput instead of gaining 2.5 (profiles/side_stream/).  Three batch handles open three
// main and three side streams beside the context's own, so the library asks for ARX_HW_QUEUES (8) when it is loaded, by raising the variable
// where it is unset or lower, never above 32.  The runtime reads the variable once, when it is initialised: a process that has opened the
// GPU before it loads the library (the HSA runtime holds /dev/kfd open from then on) keeps the queues it has.  So the request also records
// whether the side streams will have their queues, and ARX_AUX_STREAM's default follows that: on where the variable already was high enough
// or the request came in time, off (one stream per batch, the order before the side streams) in a process that had the GPU open with fewer.
// ARX_HW_QUEUES=0, or ARX_AUX_STREAM=0 at load time, makes no request.  setenv is not safe against a getenv in another thread at the same
// moment; the request runs once, in the loader's call of the library's constructors.
inline bool sw_gpu_already_open() // does a descriptor of this process name /dev/kfd?  (no /proc: taken as not open)
{
	DIR *d = opendir("/proc/self/fd");
	if (!d) return false;
	bool open = false;
	while (const dirent *e = readdir(d)) {
		char to[64];
		const ssize_t n = readlinkat(dirfd(d), e->d_name, to, sizeof to - 1);
		if (n == 8 && memcmp(to, "/dev/kfd", 8) == 0) { open = true; break; }
	}
	closedir(d);
	return open;
}
inline bool &sw_side_streams_have_queues() { static bool have = false; return have; } // per loaded library; false until the request has run
inline void sw_request_hw_queues()
{
	bool &have = sw_side_streams_have_queues();
	int need = sw_int("ARX_HW_QUEUES", 8);
	if (need > 32) need = 32;
	const char *e = getenv("GPU_MAX_HW_QUEUES");
	if (e && atoi(e) >= (need > 0 ? need : 8)) { have = true; return; } // (as the process was started: taken to be what the runtime read or will read)
	have = false;
	if (need <= 0 || !sw_on_unless_zero("ARX_AUX_STREAM") || sw_gpu_already_open()) return;
	char v[16];
	snprintf(v, sizeof v, "%d", need);
	have = setenv("GPU_MAX_HW_QUEUES", v, 1) == 0;
}
inline bool sw_aux_stream() { const char *e = getenv("ARX_AUX_STREAM"); return e ? atoi(e) != 0 : sw_side_streams_have_queues(); } // set: as it says (1 forces the side streams); unset: where they have their queues

// ---- batch switches: everything the runtime (hip_rt.h, arx_cold.hip) looks at
struct BatchSwitches {
	// -- streams and launch shapes
	// The side stream (HipRT::on_aux): launches that keep a few wavefronts busy run beside the wide launch of the same stage instead of in
	// front of it.  ARX_AUX_STREAM is the master switch (0: every launch on the batch's one stream; unset: on where the side streams have
	// their hardware queues, sw_request_hw_queues above); each part has its own beneath it.
	// Round 2 measured the side stream as a loss with three batches in flight (7.1 against 7.6 M pairs/s); profiles/side_stream/ has that
	// measurement again with enough hardware queues for the streams (sw_request_hw_queues above) and the A/B of each part.
	// A part is on by default where every run with it was faster than every run without it (three runs each, alternating, the default bench
	// command; the table is in profiles/side_stream/README.md): the chaining fork and the rescue replay are, the others are not.
	bool aux_stream = sw_aux_stream();
	bool aux_chain = sw_on_unless_zero("ARX_AUX_CHAIN");         // KChainMid (the above-cap reads' walk) beside both k_chain_heavy launches: 74.7-75.1 -> 73.4-74.1 ms per step
	bool aux_rescue = sw_on_unless_zero("ARX_AUX_RESCUE");       // k_rescue_heavy beside the thread-per-pair launch of its round (round 2's part): 73.4-74.1 -> 72.8-73.4
	bool aux_dedup = sw_off_unless_nonzero("ARX_AUX_DEDUP");     // k_dedup_heavy beside KDedup, after a pass of its own that lists the heavy reads
	bool aux_nw = sw_off_unless_nonzero("ARX_AUX_NW");           // CIGAR band class 2 beside the other classes
	// 8 resident 64-thread blocks per CU give every SIMD two waves of these latency-bound kernels
	int bpc = sw_int("ARX_BPC", 16);                       // resident 64-lane blocks per CU of the thread-per-item kernels (sizes their per-slot scratch)
	int coop_bpc = sw_int("ARX_COOP_BPC", 64);             // grid cap of the 16-lane DP kernels (no per-slot scratch; grid-stride)
	int ext_merge_below = sw_int("ARX_EXT_MERGE", 30000);  // rounds with fewer extensions run all length classes in one launch
	bool wide = sw_on_unless_zero("ARX_WIDE");             // 0: launch_wide falls back to the capped grid-stride launch (A/B)
	bool ext_old = sw_off_unless_nonzero("ARX_EXT_OLD");   // A/B: round 2's extension kernel (ext2_g16) on the same class lists
	// rescue SW: ARX_SW_SIMPLE selects the one-thread-per-item kernels everywhere (A/B runs).  Quirk: present means on, so ARX_SW_SIMPLE=0 is ON
	bool sw_simple = sw_present("ARX_SW_SIMPLE");
	// Off by default: on the benchmark workload 99.6 % of the rescue alignments are real hits in repeat copies (nothing to drop, the
	// filter's 1 ms per batch is lost); on workloads with chimeric or unpaired reads it drops 40 % of them (profiles/r01/README.md).
	int sw_filter = sw_int("ARX_SW_FILTER", 0);
	int sw_filter_stats = sw_int("ARX_SW_FILTER_STATS", 0); // diagnostics: one extra host round trip per launch
	// -- seeding (hip_fm_coop.h).  seed_bpc / strat_bpc unset: 4 * ARX_SEED_WPE resident blocks per CU (the kernels' register budget is compiled
	// for that many waves per SIMD; the macro is hip_fm_coop.h's, so the runtime supplies the default)
	std::optional<int> strat_bpc = sw_int_if_set("ARX_STRAT_BPC"); // resident blocks per CU of the third seeding pass
	std::optional<int> seed_bpc = sw_int_if_set("ARX_SEED_BPC");
	int seed_bwd_mid = sw_int("ARX_SEED_BWD_MID", 21);         // longest list of the 21-lane bin of the backward sweeps (16: none)
	int seed_bwd_e_bpc = sw_int("ARX_SEED_BWD_E_BPC", 32);     // resident workgroups per CU of the entry-parallel sweeps (62 VGPRs: eight wavefronts per SIMD fit)
	int seed_bwd_e_chunk = sw_int("ARX_SEED_BWD_E_CHUNK", 256); // list entries a wavefront reserves per atomic (entry-parallel sweeps)
	bool seed_fit32 = sw_on_unless_zero("ARX_SEED_FIT32");     // 0: the general (40-bit) arithmetic in the backward sweeps whatever the index (A/B)
	bool text_bwd = sw_on_unless_zero("ARX_TEXT_BWD");         // 0: every sweep walked to its end (k_seed_bwd_g hands nothing to KSeedBwdTail)
	// the row-parallel backward kernel needs 94 VGPRs: five wavefronts per SIMD fit, not only the four its launch bound asks for, so its grid is
	// 20 workgroups per CU (4.81 -> 4.62 ms alone; 24 and more lose again, and a build that forces six per SIMD spills: 7.2 ms)
	int seed_bwd_bpc = sw_int("ARX_SEED_BWD_BPC", 20);
	int seed_batch = sw_int("ARX_SEED_BATCH", 48);             // lanes that queue up before the slow bookkeeping runs
	int seed_bwd_budget = sw_int("ARX_SEED_BWD_BUDGET", 128);  // extensions a lane spends on one backward sweep before handing it to a wavefront (0: never)
	int seed_chunk = sw_int("ARX_SEED_CHUNK", 64);             // items a wavefront reserves per atomic
	// backward sweeps vary most in length: smaller reservations even out the end of the launch (64: 10.3 ms, 32: 9.4, 16: 9.7, 8: 10.3 per batch).
	// Quirk: unset, it falls back to ARX_SEED_CHUNK when that is set, and only then to 32
	int seed_bwd_chunk = sw_int("ARX_SEED_BWD_CHUNK", sw_int("ARX_SEED_CHUNK", 32));
	// Backward sweeps: 2 (default) = row-parallel, one task per 16/32/64-lane group with the row's entries in registers (k_seed_bwd_g<GL>,
	// tasks binned by list length): 21.5 -> 10 ms per 667 k-read batch at GRCh38 size.  1 = the pipelined one-lane-per-task kernel
	// k_seed_bwd2 (51-61 of 64 lanes extending instead of 25-32, but no faster: profiles/r02/README.md).  0 = round 1's k_seed_bwd.
	// 3 = entry-parallel (k_seed_bwd_e).  All four are held to the CPU restatement interval for interval (tests/test_seed_variants_gpu.py).
	int seed_bwd2 = sw_int("ARX_SEED_BWD2", 2);
	int seed_grant = sw_int("ARX_SEED_GRANT", 4);              // first forward pass: lanes parked for a pool slice that trigger the hand-out (5.36 ms with none, 5.17 at 16, 4.94 at 4, 5.08 at 1)
	int seed_bwd_batch = sw_int("ARX_SEED_BWD_BATCH", 0);      // 0: seed_batch
	// 0: the thread-per-read forms of the list passes seed_merge and occ_fill (KSeedMerge, KOccFill) instead of the 16-lane group forms of
	// hip_seed_lists.h (A/B, and the test that holds the two forms together: tests/test_seed_lists_gpu.py)
	bool seed_lists = sw_on_unless_zero("ARX_SEED_LISTS");
	// -- heavy-item kernels (arx_cold.hip)
	bool rescue_heavy = sw_on_unless_zero("ARX_RESCUE_HEAVY"); // 0: no wavefront replay of the pairs with long lists (A/B)
	bool chain_heavy = sw_on_unless_zero("ARX_CHAIN_HEAVY");   // 0: no wavefront-per-read chaining of the reads with many occurrences (A/B)
	bool dedup_heavy = sw_on_unless_zero("ARX_DEDUP_HEAVY");   // 0: no wavefront-per-read de-duplication of long region lists (A/B)
	// opt-in (ARX_CHAIN_GROUP=1): chaining of the reads below the heavy kernel's threshold, one 16-lane group per read on a working set in LDS
	// (arx_cold.hip: k_chain_g16).  Default: every such read is chained by its own thread in HBM (KChain / KChainMid) -- the group form
	// measured no faster (profiles/chain_group/)
	bool chain_group = sw_off_unless_nonzero("ARX_CHAIN_GROUP");
	int rescue_wave = sw_int("ARX_RESCUE_WAVE", 1);            // 0: lane 0 alone replays a heavy pair (A/B of k_rescue_heavy's wavefront form)
	// 1: three launches by LDS footprint (170 / 340 / 680 records: 5 / 3 / 2 workgroups per CU).  Measured in round 3: slower (36 -> 43 ms per step
	// alone on the repeat-rich workload, 14 -> 18 on the default one) -- the launches of one stream run one after the other and each ends on
	// its own longest pair; what bounds this kernel is the serial depth of its longest pairs, not the workgroups a CU holds.  Default: one launch.
	int rescue_lds_classes = sw_int("ARX_RESCUE_LDS_CLASSES", 0);
	int chain_wave = sw_int("ARX_CHAIN_WAVE", 1);              // 0: lane 0 alone runs chain_and_filter() in k_chain_heavy (A/B)
	int chain_l_div = sw_int("ARX_CHAIN_L_DIV", 1);            // the long ones' launch holds 128 KB of LDS per workgroup: on n_cu / l_div CUs
	// -- workgroup-per-item kernels (hip_block.h: launch_block)
	// largest P that sort_kv orders by counting ranks (one entry per lane, 2 barrier phases) instead of by the bitonic network; never above the
	// class's lane count.  Unset: hip_block.h's RANK_SORT_MAX / SMALL_RANK_SORT_MAX, both 0 (the bitonic network for every P): the rank sort
	// measured 2.3 to 6.7 times slower than the network at P = 256 to 1,024 (P * P comparisons; profiles/rfa_sweeps/)
	std::optional<int> block_rank_sort = sw_int_if_set("ARX_BLOCK_RANK_SORT");
	// -- diagnostics
	bool trace_launches = sw_present("ARX_TRACE_LAUNCHES");    // name every launch on stderr and wait for it (a fault then names its kernel)
	bool seed_stats = sw_present("ARX_SEED_STATS");            // lane utilisation of the persistent-lane seeding kernels, printed per launch
	bool seed_hist = sw_present("ARX_SEED_HIST");              // forward-list lengths of every backward launch's tasks
};

// ---- pipeline switches: what the stages themselves look at (pipeline.h, pipeline_rfa.h), none of them the runtime's business
struct PipelineSwitches {
	// -- seeding
	// reads per pass through the first two seeding passes (0: the whole batch at once; groups shrink the interval pool from 12 KB to 12 KB x
	// group / batch per read at the price of under-filled forward launches: 0 / 360 k / 180 k / 90 k reads -> 7.0 / 9.5 / 11.4 / 14.1 ms of
	// seed_fwd per 667 k-read batch, seed_bwd unchanged)
	int seed_group_reads = sw_int("ARX_SEED_GROUP", 0);
	int seed_tasks_per_read = sw_int("ARX_SEED_TASKS", 12);    // seeding tasks per read (all three passes), same rule
	int seed_pool_per_read = sw_int("ARX_SEED_POOL", 384);     // interval-pool entries per read (3 per forward-list entry); an overflow is reported, never silent
	bool seed_bwd_entry = sw_present("ARX_SEED_BWD_ENTRY");    // KSeedBwd entry by entry (only the one-thread form looks at it: the host test double, ARX_SW_SIMPLE)
	// -- thresholds of the heavy-item kernels; *_heavy_min unset: pipeline.h's CHAIN_HEAVY_MIN / DEDUP_HEAVY_MIN / RESCUE_HEAVY_MIN
	std::optional<int> chain_heavy_min = sw_int_if_set("ARX_CHAIN_HEAVY_MIN");   // occurrences from which a read is heavy (tests lower it; raised, k_chain_g16's LDS opt-in goes above 64 KB)
	std::optional<int> dedup_heavy_min = sw_int_if_set("ARX_DEDUP_HEAVY_MIN");   // regions from which a read is heavy (tests)
	std::optional<int> rescue_heavy_min = sw_int_if_set("ARX_RESCUE_HEAVY_MIN"); // regions of both reads together from which a pair is heavy (tests)
	// beneath ARX_AUX_CHAIN: the classification of the reads as a pass of its own (KChainClass), then the light reads' chaining, KChainMid and
	// the k_chain_heavy launches all three side by side (two side streams).  Off: 74.2-74.5 ms per step with it against 73.4-74.1 without
	// (the seed phase of the batches beside it grows by more than the align phase shrinks)
	bool chain_split = sw_off_unless_nonzero("ARX_CHAIN_SPLIT");
	int chain_mid_min = sw_int("ARX_CHAIN_MID_MIN", 16);       // occurrences from which a read below the heavy threshold is listed for KChainMid; 0: no launch of their own for the reads in between
	bool rescue_no_ahead = sw_present("ARX_RESCUE_NO_AHEAD");  // every rescue SW down the one-at-a-time path instead of queued ahead (tests)
	// -- extension
	// 0: every extension task goes to the DP.  Default: KExtStep answers the tasks their diagonal decides itself (dev_sw.h ext_closed_form: at
	// most one differing pair, no ambiguous base, h0 >= 5, tlen >= qlen) and the chain goes on in the same round (profiles/ext_closed/)
	bool ext_closed = sw_on_unless_zero("ARX_EXT_CLOSED");
	// -- placement (pipeline_rfa.h)
	// Barcodes of TELLseq size (at most 512 reads and 512 candidates) in 256-lane workgroups, ten per CU instead of two (hip_block.h);
	// ARX_RFA_SMALL=0: 1,024 lanes for every barcode.  Round 2 measured the small class as a loss (23.3 ms against 7.4 ms per batch of 4,333
	// barcodes x 77 pairs): a barcode was a chain of about a hundred barrier phases whose length grew with the work per lane.  With the idle
	// sweeps gone (rfa_skip_sweeps below) the chain is a third shorter and the verdict turns: 70.7-71.5 ms per step with the small class against
	// 71.9-72.5 without, eight alternating runs each, every run with it faster than every run without (profiles/rfa_sweeps/).  Default: on.
	bool rfa_small = sw_on_unless_zero("ARX_RFA_SMALL");
	// 0: the placement walk (R5) and the move sums (R6) sweep every source molecule.  Default: only the sources that hold a read with spots in
	// two or more molecules -- no other sweep can add anything (dev_rfa.h states the rule); the results are the same bit for bit
	// (tests/test_rfa_sweeps_hostsim.py, tests/test_rfa_sweeps_gpu.py hold the two forms together).  Measurement: profiles/rfa_sweeps/
	bool rfa_skip_sweeps = sw_on_unless_zero("ARX_RFA_SKIP_SWEEPS");
	std::optional<double> mapq_guard = sw_double_if_set("ARX_MAPQ_GUARD"); // unset: dev_rfa.h's RFA_MAPQ_GUARD; tests widen the guard to push every read through the host path
	// -- diagnostics
	bool trace = sw_present("ARX_TRACE");                      // per-round progress on stderr
	bool seed_dump = sw_present("ARX_SEED_DUMP");              // the first-pass tasks of the first reads and their forward lists
};

// ---- feeder switches (device_feeder.h)
struct FeederSwitches {
	// chunks a parse takes from each file (default: as many as fill SLAB_TARGET, at most 64); 1 makes every chunk boundary a boundary between
	// parses.  Quirk: a value below 1, or one whose chunks together exceed MAX_CHUNK, is ignored without a word (DeviceFeeder::open)
	std::optional<long> parse_chunks = sw_long_if_set("ARX_FEEDER_PARSE_CHUNKS");
	// the gzip inflate of ARX_FEEDER_GUNZIP_DEVICE: compressed bytes per chunk (default: gunzip_host.h's GZ_CHUNK_DEFAULT) and per launch (default:
	// the rule at the top of device_feeder.h).  Tests put many chunks and launches into a small file with them; a value outside
	// arx_selftest_gunzip's bounds makes the open fail (ARX_E_ARG)
	std::optional<long> gunzip_chunk = sw_long_if_set("ARX_FEEDER_GUNZIP_CHUNK");
	std::optional<long> gunzip_slab = sw_long_if_set("ARX_FEEDER_GUNZIP_SLAB");
	bool times = sw_present("ARX_FEEDER_TIMES");               // diagnostics: where the feeder thread's time went, and the kernels' own times (HIP events)
};

// ---- the one per-process switch.  ARX_LAUNCH_LOG names a file that every runtime of the process appends one line per launch to (name, items,
// ms) through one static FILE * (HipRT::resolve_timers): it is opened once, the first time a runtime resolves its timers, and a change of the
// variable after that goes unseen.  Diagnostics.
inline FILE *sw_open_launch_log() { const char *e = getenv("ARX_LAUNCH_LOG"); return e ? fopen(e, "a") : nullptr; }

// ---- the parts of the side stream (HipRT::on_aux): which switch of BatchSwitches, beneath ARX_AUX_STREAM, a fork belongs to
enum AuxPart { AUX_RESCUE, AUX_CHAIN, AUX_DEDUP, AUX_NW };

} // namespace arx

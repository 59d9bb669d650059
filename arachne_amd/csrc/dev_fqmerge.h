// dev_fqmerge.h -- the FASTQ sort of dev_fqsort.h for a file pair that device memory does not hold: sorted runs, and their merge on the device.
// As dev_fqsort.h it is shared by the kernels' driver (hip_fqsort.h) and the host program (tests/fqextsim/fastq_sort_ext_sim.cpp).
//
// Runs.  Two device buffers of run_bytes take the next bytes of the two files behind what the run before left over (the carry).  The buffers
// are parsed as a part of their files (fs_parse_part): where a buffer's end is not its file's end the parse stops there, and the line pairs
// behind the last record that is whole in both buffers move to the buffers' fronts.  The two carries differ in size as the files' line lengths
// do; each buffer is filled up to run_bytes whatever its carry was.  The end-of-input rule is applied once, by the parse that meets a file's
// end.  A run's records are ordered and gathered as an in-core sort's (fs_order, fs_gather) and appended to the two run files through `io`.
// A run in which not one line pair could be consumed although a buffer was full is FS_E_RUN; more than FS_MAX_RUNS runs are FS_E_RUNS.
//
// Keys.  Every record of a sorted run gets a row of the global table (FxKeepF): where it lies in the two run files, and its barcode, copied
// into one compact key buffer.  The table is run-major and sorted within a run, so a STABLE sort of it by barcode is the input-stable global
// order: equal barcodes fall in run order, within a run in the run's order, which is input order.  fs_order over (key buffer, global table)
// is that sort, and the output's prefix sums.  The input's barcode runs are the runs' own less one per barcode that continues over a border.
//
// Merge.  An output slab is a range [j0, j1) of the global order.  Its records from run r are a contiguous range of run r's rows (the stable
// sort keeps a run's rows in their order), found by two binary searches per run over the inverse permutation (FxRangeF: nothing depends on
// the order of the items).  The rows' bytes are contiguous in the run files too: the host reads exactly these ranges into the stage buffers,
// which thereby hold exactly the slab's bytes, and FxGatherF copies every record from there to its place, FS_GATHER_LANES lanes per record
// and file.  A run's ranges move forward from slab to slab: each run file is read once, front to back.
//
// Beyond dev_fqsort.h's the driver supplies
//     drv.run_buf(f, bytes)              the run buffer of file f
//     drv.copy(dst, src, n)              n bytes within launch memory, not overlapping
//     drv.upload(dev, host, bytes)       host memory to launch memory; the host's may be reused on return
//     drv.keep(which, bytes, kept)       growing memory (0: the global table, 1: the key buffer) with room for `bytes`, its first `kept` bytes staying
// the source  src.fill(f, dst, want) -> the bytes put at dst, fewer than `want` only at the file's end; src.ended(f): nothing is left of file f
// and io      take / give (a sink of fs_gather: the slabs of a run, appended to the run files), end_run(), and for the merge
//             begin(bytes) (so many bytes will be read for a slab), read(f, at, n, dst) (bytes [at, at + n) of run file f to launch memory), staged()
//
// Memory per record of the whole input: the global table's 40 bytes and the barcode throughout; 40 more while the merge orders (two key and two
// value arrays, two arrays of output offsets).  Per run: the two buffers and a run's own 80 bytes per record.
#pragma once
#include <string>
#include <vector>
#include "dev_fqsort.h"

namespace arx {

constexpr int64_t FS_MAX_RUNS = 1024; // the runs of one sort: every slab of the merge asks every run for its range
enum { FS_E_RUN = 3, FS_E_RUNS = 4, FS_E_MERGE = 5 };

template <class K> struct FxKeyLenF {
	K key; const uint32_t *vals; int64_t *len;
	ARX_DEVI void operator()(int64_t j) const { len[j] = key.len(vals[j]); }
};
// place j of a sorted run -> row j of the run's rows in the global table; the key byte by byte through its accessor (dev_fqsort.h): it has no
// length cap and no alignment, and need not lie in one piece
template <class K> struct FxKeepF {
	K key; const uint32_t *vals; const int64_t *out1, *out2, *koff; int64_t file1, file2, key0; FsRec *rows; uint8_t *keys;
	ARX_DEVI void operator()(int64_t j) const
	{
		const int64_t row = vals[j], n = key.len(row);
		FsRec o;
		o.off1 = file1 + out1[j]; o.len1 = (int32_t)key.size1(row);
		o.off2 = file2 + out2[j]; o.len2 = (int32_t)key.size2(row);
		o.bc_off = key0 + koff[j]; o.bc_len = (int32_t)n; o.pad = 0;
		rows[j] = o;
		for (int64_t k = 0; k < n; ++k) keys[o.bc_off + k] = key.byte(row, k);
	}
};
struct FxInvF {
	const uint32_t *vals; uint32_t *inv;
	ARX_DEVI void operator()(int64_t j) const { inv[vals[j]] = (uint32_t)j; }
};
// the first row g in [lo, hi) whose place in the order is j or later (a run's rows keep their order: inv ascends over them)
ARX_DEVI int64_t fx_rank(const uint32_t *inv, int64_t lo, int64_t hi, int64_t j)
{
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo) / 2;
		if ((int64_t)inv[mid] < j) lo = mid + 1; else hi = mid;
	}
	return lo;
}
// item: a run.  range[6 r ..]: its rows in the slab [j0, j1), and their bytes in the two run files
struct FxRangeF {
	const FsRec *rows; const uint32_t *inv; const int64_t *first; int64_t j0, j1; int64_t *range;
	ARX_DEVI void operator()(int64_t r) const
	{
		const int64_t lo = fx_rank(inv, first[r], first[r + 1], j0), hi = fx_rank(inv, lo, first[r + 1], j1);
		int64_t *o = range + 6 * r;
		o[0] = lo; o[1] = hi;
		o[2] = o[3] = o[4] = o[5] = 0;
		if (hi > lo) { o[2] = rows[lo].off1; o[3] = rows[hi - 1].off1 + rows[hi - 1].len1; o[4] = rows[lo].off2; o[5] = rows[hi - 1].off2 + rows[hi - 1].len2; }
	}
};
struct FxGatherF { // FsGatherF from the stage buffers: delta[2 r + f] moves an offset in run file f to the stage buffer, for the rows of run r
	const uint8_t *s1, *s2; const FsRec *rows; const uint32_t *vals; const int64_t *out1, *out2, *first, *delta; int64_t n_runs, j0; uint8_t *d1, *d2;
	ARX_DEVI void operator()(int64_t i) const
	{
		const int lane = (int)(i % FS_GATHER_LANES);
		const bool two = (i / FS_GATHER_LANES) & 1;
		const int64_t j = j0 + i / (2 * FS_GATHER_LANES), g = vals[j];
		int64_t lo = 0, hi = n_runs - 1; // the run r with first[r] <= g < first[r + 1]
		while (lo < hi) {
			const int64_t mid = lo + (hi - lo + 1) / 2;
			if (first[mid] <= g) lo = mid; else hi = mid - 1;
		}
		const FsRec &r = rows[g];
		if (two) bs_copy(d2 + (out2[j] - out2[j0]), s2 + (r.off2 + delta[2 * lo + 1]), r.len2, lane, FS_GATHER_LANES);
		else bs_copy(d1 + (out1[j] - out1[j0]), s1 + (r.off1 + delta[2 * lo]), r.len1, lane, FS_GATHER_LANES);
	}
};

struct FxRuns {
	int64_t N = 0, key_bytes = 0, n_runs = 0, file1 = 0, file2 = 0, runs_in = 0, skipped = 0, windows = 0;
	std::vector<int64_t> first;    // first[r]: run r's first row of the global table; first[n_runs] = N
	std::vector<uint8_t> last_bc;  // the barcode of the last record so far, in input order
	FsRec *rows = nullptr;         // the global table
	uint8_t *keys = nullptr;
};

// [at, at + n) of b to its front: forward, in pieces that do not overlap their destination
template <class Drv> void fx_to_front(Drv &drv, uint8_t *b, int64_t at, int64_t n)
{
	if (at == 0) return;
	for (int64_t done = 0; done < n; done += at) drv.copy(b + done, b + at + done, n - done < at ? n - done : at);
}
template <class Drv> std::vector<uint8_t> fx_barcode(Drv &drv, const uint8_t *t1, const FsRec *rec)
{
	FsRec r;
	drv.fetch(&r, rec, sizeof r);
	std::vector<uint8_t> b((size_t)r.bc_len);
	if (r.bc_len) drv.fetch(b.data(), t1 + r.bc_off, (size_t)r.bc_len);
	return b;
}
// what a run's records are to the sort: their key accessor, their gather, a key read by the host.  These are arx_fastq_sort's; dev_fqprep.h has
// the ones of records whose header is composed on the way
struct FxPlainRows {
	template <class Drv> FsPlainKey key(Drv &, const FsText &T, const FsRec *tab, int64_t, FsSortMem &) { return FsPlainKey{T.t1, tab}; }
	template <class Drv, class Sink> void gather(Drv &drv, const FsText &T, const FsPlainKey &key, int64_t n, const FsSortMem &m, int64_t slab, int64_t longest, Sink &sink, FsCounts &c)
	{
		fs_gather(drv, T, key.tab, n, m, slab, longest, sink, c);
	}
	template <class Drv> std::vector<uint8_t> key_bytes(Drv &drv, const FsPlainKey &key, int64_t row) { return fx_barcode(drv, key.t1, key.tab + row); }
};

// the runs: parsed, ordered, (io != null) appended to the run files, their keys kept.  FS_OK, or FS_E_*
template <class Drv, class Src, class Io, class Rows> int fx_runs_by(Drv &drv, Src &src, Io *io, int64_t run_bytes, int64_t window, int64_t slab, FxRuns &S, Rows &rows)
{
	uint8_t *buf[2] = {(uint8_t *)drv.run_buf(0, run_bytes), (uint8_t *)drv.run_buf(1, run_bytes)};
	int64_t have[2] = {0, 0};
	S = FxRuns();
	S.first.assign(1, 0);
	for (;;) {
		for (int f = 0; f < 2; ++f)
			if (!src.ended(f) && have[f] < run_bytes) have[f] += src.fill(f, buf[f] + have[f], run_bytes - have[f]);
		const FsText T = {buf[0], buf[1], have[0], have[1]};
		FsPart p;
		p.open1 = !src.ended(0); p.open2 = !src.ended(1); p.n_before = S.N;
		FsCounts cr{};
		if (const int rc = fs_parse_part(drv, T, window, cr, p)) return rc;
		S.skipped += cr.skipped; S.windows += cr.windows;
		if (!p.ended && p.lines == 0) return FS_E_RUN; // a buffer is full, and the parse could not leave its front
		const int64_t n = cr.n_records;
		if (n > 0) {
			if (S.n_runs == FS_MAX_RUNS) return FS_E_RUNS;
			const FsRec *tab = drv.table(n);
			FsSortMem m;
			fs_sort_mem(drv, n, m);
			const auto key = rows.key(drv, T, tab, n, m);
			typedef decltype(rows.key(drv, T, tab, n, m)) K;
			const int64_t longest = fs_order_by(drv, key, n, m, cr);
			const std::vector<uint8_t> head = rows.key_bytes(drv, key, 0);
			S.runs_in += cr.runs_in - (S.n_runs > 0 && head == S.last_bc ? 1 : 0);
			S.last_bc = rows.key_bytes(drv, key, n - 1);
			if (io) {
				rows.gather(drv, T, key, n, m, slab, longest, *io, cr);
				io->end_run();
			}
			int64_t *koff = (int64_t *)drv.work(FS_W_KOFF, 8 * (n + 1));
			drv.items("fx_key_len", n, FxKeyLenF<K>{key, m.vals[m.cur], (int64_t *)m.keys[0]});
			drv.scan((const int64_t *)m.keys[0], koff, n);
			const int64_t kb = drv.get(&koff[n]);
			S.rows = (FsRec *)drv.keep(0, (S.N + n) * (int64_t)sizeof(FsRec), S.N * (int64_t)sizeof(FsRec));
			S.keys = (uint8_t *)drv.keep(1, S.key_bytes + kb, S.key_bytes);
			drv.items("fx_keep", n, FxKeepF<K>{key, m.vals[m.cur], m.out1, m.out2, koff, S.file1, S.file2, S.key_bytes, S.rows + S.N, S.keys});
			S.N += n; S.key_bytes += kb; S.file1 += cr.bytes1; S.file2 += cr.bytes2;
			++S.n_runs;
			S.first.push_back(S.N);
		}
		if (p.ended) return FS_OK;
		fx_to_front(drv, buf[0], p.a1, have[0] - p.a1); have[0] -= p.a1;
		fx_to_front(drv, buf[1], p.a2, have[1] - p.a2); have[1] -= p.a2;
	}
}
template <class Drv, class Src, class Io> int fx_runs(Drv &drv, Src &src, Io *io, int64_t run_bytes, int64_t window, int64_t slab, FxRuns &S)
{
	FxPlainRows rows;
	return fx_runs_by(drv, src, io, run_bytes, window, slab, S, rows);
}

// the global order, the counts of the whole input, and (sink != null) the output, slab by slab as fs_gather makes it
template <class Drv, class Io, class Sink> int fx_merge(Drv &drv, Io *io, Sink *sink, const FxRuns &S, int64_t slab_bytes, FsSortMem &m, FsCounts &c)
{
	const int64_t N = S.N, R = S.n_runs;
	fs_sort_mem(drv, N, m);
	const FsText K = {S.keys, nullptr, S.key_bytes, 0};
	const int64_t longest = fs_order(drv, K, S.rows, N, m, c);
	c.n_records = N; c.skipped = S.skipped; c.windows = S.windows; c.runs_in = S.runs_in; c.slabs = 0;
	if (!sink || N == 0) return FS_OK;
	const uint32_t *vals = m.vals[m.cur];
	uint32_t *inv = m.vals[m.cur ^ 1];
	drv.items("fx_inv", N, FxInvF{vals, inv});
	int64_t *first = (int64_t *)drv.work(FS_W_FIRST, 8 * (R + 1)), *range = (int64_t *)drv.work(FS_W_RANGE, 48 * R), *delta = (int64_t *)drv.work(FS_W_DELTA, 16 * R);
	drv.upload(first, S.first.data(), (size_t)(8 * (R + 1)));
	std::vector<int64_t> hr((size_t)(6 * R)), hd((size_t)(2 * R));
	const int64_t cap = slab_bytes > longest ? slab_bytes : longest;
	int64_t at1 = 0, at2 = 0;
	for (int64_t j0 = 0; j0 < N;) {
		int64_t lo = j0 + 1, hi = N; // fs_gather's slab
		while (lo < hi) {
			const int64_t mid = lo + (hi - lo + 1) / 2;
			if (drv.get(&m.out1[mid]) - at1 <= slab_bytes && drv.get(&m.out2[mid]) - at2 <= slab_bytes) lo = mid; else hi = mid - 1;
		}
		const int64_t e1 = drv.get(&m.out1[lo]), e2 = drv.get(&m.out2[lo]), b[2] = {e1 - at1, e2 - at2};
		drv.items("fx_range", R, FxRangeF{S.rows, inv, first, j0, lo, range});
		drv.fetch(hr.data(), range, (size_t)(48 * R));
		uint8_t *stage[2] = {(uint8_t *)drv.work(FS_W_STAGE1, b[0]), (uint8_t *)drv.work(FS_W_STAGE2, b[1])};
		io->begin(b[0] + b[1]);
		int64_t base[2] = {0, 0};
		for (int64_t r = 0; r < R; ++r)
			for (int f = 0; f < 2; ++f) {
				const int64_t from = hr[(size_t)(6 * r + 2 + 2 * f)], n = hr[(size_t)(6 * r + 3 + 2 * f)] - from;
				hd[(size_t)(2 * r + f)] = base[f] - from;
				if (n <= 0) continue;
				if (base[f] + n > b[f]) return FS_E_MERGE;
				io->read(f, from, n, stage[f] + base[f]);
				base[f] += n;
			}
		if (base[0] != b[0] || base[1] != b[1]) return FS_E_MERGE; // the staged bytes of a slab are exactly the slab's bytes
		io->staged();
		drv.upload(delta, hd.data(), (size_t)(16 * R));
		uint8_t *d1 = nullptr, *d2 = nullptr;
		sink->take(c.slabs, cap, b[0], b[1], &d1, &d2);
		drv.items("fx_gather", (lo - j0) * 2 * FS_GATHER_LANES, FxGatherF{stage[0], stage[1], S.rows, vals, m.out1, m.out2, first, delta, R, j0, d1, d2});
		sink->give(c.slabs, j0, lo, b[0], b[1]);
		++c.slabs;
		j0 = lo; at1 = e1; at2 = e2;
	}
	return FS_OK;
}

} // namespace arx

// hip_fqsort.h -- dev_fqsort.h on the GPU, and the driver behind arx_fastq_sort and arx_selftest_fastq_sort (arx_bgzf.hip): a FASTQ file pair
// sorted by barcode, the reference's `preprocess` (src/preprocess/preprocess.go:42-114: samtools import | sort -t BX | fastq) without samtools.
//
//   k_fs_items<F>    one item of a functor of dev_fqsort.h (or, wrapped, of dev_fastq.h) per thread, started through hip_launch under the
//                    functor's name.  An item is a 16-byte word (window, newlines), a block of line pairs (state scan), a record (fields, table,
//                    keys, runs, sizes) or one of the FS_GATHER_LANES lanes of a record of one file (gather)
// The key sorts are rocprim::radix_sort_pairs over the bits that differ, the prefix sums rocprim's scan, the maximum and the OR rocprim's reduce.
// The streams, events, every buffer and rocprim's scratch are owners of hip_res.h.
//
// The files.  Each input is judged by its own first bytes: a BGZF file is read as it is, slab by slab (BgzfChunkReader), and inflated on the device
// (inflate_launch: only compressed bytes go up); anything else -- plain text, ordinary gzip -- goes through zlib on a reader thread (ChunkReader).
// With ARX_FQSORT_GUNZIP_DEVICE (ARX_FQSTD_GUNZIP_DEVICE) an ordinary gzip file (file_is_gzip) is read as it is too (GzipRawReader) and inflated
// on the device in chunks (FsGunzip: gunzip_host.h's reader over hip_gunzip.h): its size is known only after the decode pass, so such a file
// comes in two steps -- the size of the next piece, then room() or the caller's place, then the resolve straight into it.
// Host memory holds two slabs per file, never a file.  The inflated texts of both files stay in device memory until the call ends.
// The output leaves in slabs of FS_SLAB_DEFAULT bytes per file from two pairs of buffers: while slab k is fetched and written (plain text), or
// compressed and written (ARX_FQSORT_BGZF: DeviceBgzf::run_device, blocks cut every 65280 bytes, the 28-byte EOF block last), slab k + 1 is
// gathered.  It goes to <out>.tmp, renamed when everything is written and removed otherwise.
//
// The host side is one path, shared with arx_fastq_standardize and arx_fastq_prepare (hip_fqstd.h, hip_fqprep.h).  In: FsInput::open and
// fs_open_inputs / fs_probe_inputs; FxFileSrc::take acquires a reader's slab, checks it and has FsSlabUp bring it up to where its caller
// points -- next(): the source's own slab text, which fills runs and windows; load(): its place in the whole text, no copy between.  Out:
// FsFileSink::open / begin / end (both <out>.tmp, whose names a failed fopen forgets, so that nothing is removed that the call did not create;
// the compressor; finish() with its times booked) and FxFileStore::create (the run files).  In core: fs_run_by over a row policy, as fx_run_by
// for runs.  What is refused is thrown (FsBadArg, FsTooLarge, FsIoError) and becomes code and text in arx_bgzf.hip's fq_file_call.
//
// Device memory of a call: the two texts (a text that outgrows its buffer moves to one half as large again), four output slab buffers (256 MiB at
// the default), per record 80 bytes (dev_fqsort.h: table, keys, values, output offsets), the parse's window buffers (FS_WINDOW_DEFAULT per file,
// and about as much again for the line index), rocprim's scratch.  What does not fit is ARX_E_TOO_LARGE: sort per lane, or split the input.
//
// A pair that device memory does not hold goes through arx_fastq_sort_ex (run_bytes != 0; below: FxHipDrv ... fx_sort_files), dev_fqmerge.h on
// the GPU: the readers' slabs go up into a buffer per file and from there, split where a run ends, into the two run buffers; a run is parsed,
// ordered and gathered as above and its slabs are appended to two temporary files (FxFileStore; FxMemStore in the self-test), FxKeepF keeps a
// table row and the barcode per record; fs_order over those rows is the merge, and FxGatherF makes every output slab from the ranges of the
// runs, read back through page-locked memory.  The next slab is not staged while one is consumed: the read-back is in the open.
// Device memory of such a call.  During the runs: the two run buffers (2 run_bytes), one slab text per file as the readers cut it (32 MiB
// each), the windows and line index of a parse (min(run_bytes, FS_WINDOW_DEFAULT) per file and as much again), the run's 80 bytes per record,
// four slab buffers.  Throughout: 40 bytes and the barcode per record of the whole input (grown by half when full).  During the merge the
// runs' memory is gone: 40 bytes per record for the order, two stage buffers and four slab buffers of FS_SLAB_DEFAULT.  Not built: compressed
// run files.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_reduce.hpp>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <atomic>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/arachne_amd.h"
#include "hip_res.h"
#include "bgzf_walk.h"
#include "feeder.h"
#include "dev_fqsort.h"
#include "dev_fqmerge.h"
#include "hip_bgzf.h"
#include "hip_bamsort.h"
#include "hip_gunzip.h"

namespace arx {

constexpr int64_t FS_WINDOW_DEFAULT = (int64_t)32 << 20; // window_bytes of arx_fastq_sort
constexpr int64_t FS_SLAB_DEFAULT = (int64_t)64 << 20;   // slab_bytes of arx_fastq_sort
constexpr size_t FS_READ_CHUNK = (size_t)8 << 20;        // the readers' chunk; FS_READ_CHUNKS of them a slab
constexpr size_t FS_READ_CHUNKS = 4;
constexpr int FS_N_STATS = 20;
enum { FS_T_READ = 12, FS_T_INFLATE, FS_T_PARSE, FS_T_KEYS, FS_T_SORT, FS_T_GATHER, FS_T_COMPRESS, FS_T_WRITE };

template <class F> static __global__ void __launch_bounds__(256) k_fs_items(F f, int64_t n)
{
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n) f(i);
}

struct FsTooLarge : std::runtime_error { using std::runtime_error::runtime_error; };
struct FsIoError : std::runtime_error { using std::runtime_error::runtime_error; };
struct FsBadArg : std::runtime_error { using std::runtime_error::runtime_error; }; // what only the files show: no format to detect
struct FsOr { __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a | b; } };

constexpr const char *FS_NO_DEVICE = "no such HIP device: the FASTQ sort runs on the GPU (there is no CPU fallback)";
constexpr const char *FS_REMEDY = ": sort per lane, or split the input";

// dev_fqsort.h's driver on a stream
struct FsHipDrv {
	hipStream_t st = nullptr;
	bool timed = false;          // wait for every launch and book its time under its phase
	double us[FS_N_STATS] = {0};
	DevScratch tmp;
	DevBuf work_[FS_N_WORK], tab_, red_;
	int64_t tab_n_ = 0;

	static int phase_of(const char *nm)
	{
		if (!strncmp(nm, "fq_", 3) || !strcmp(nm, "fs_window") || !strcmp(nm, "fs_store") || !strcmp(nm, "fs_scan32")) return FS_T_PARSE;
		if (!strcmp(nm, "fs_sort")) return FS_T_SORT;
		if (!strcmp(nm, "fs_gather") || !strcmp(nm, "fs_sizes") || !strcmp(nm, "fx_gather") || !strcmp(nm, "fqs_compose") || !strcmp(nm, "fp_gather")) return FS_T_GATHER;
		return FS_T_KEYS; // length and chunk keys, runs, their scans and reductions
	}
	template <class Fn> void booked(const char *nm, Fn fn)
	{
		if (!timed) { fn(); return; }
		ARX_HIP_CHECK(hipStreamSynchronize(st));
		const double t0 = bs_now_us();
		fn();
		ARX_HIP_CHECK(hipStreamSynchronize(st));
		us[phase_of(nm)] += bs_now_us() - t0;
	}
	template <class F> void items(const char *nm, int64_t n, const F &f)
	{
		if (n <= 0) return;
		const int64_t grid = (n + 255) / 256;
		if (grid > 0x7fffffff) throw FsTooLarge(std::string("too many items for one launch") + FS_REMEDY);
		booked(nm, [&]() { hip_launch({"k_fs_items", nm}, k_fs_items<F>, dim3((unsigned)grid), dim3(256), 0, st, f, n); });
	}
	void scan(const int64_t *in, int64_t *out, int64_t n)
	{
		ARX_HIP_CHECK(hipMemsetAsync(out, 0, 8, st));
		if (n <= 0) return;
		booked("fs_scan", [&]() { dev_two_pass(tmp, "rocprim::inclusive_scan", [&](void *t, size_t &tb) { return rocprim::inclusive_scan(t, tb, in, out + 1, (size_t)n, rocprim::plus<int64_t>(), st); }); });
	}
	int64_t scan32(const int32_t *in, int32_t *out, int64_t n)
	{
		ARX_HIP_CHECK(hipMemsetAsync(out, 0, 4, st));
		if (n <= 0) return 0;
		booked("fs_scan32", [&]() { dev_two_pass(tmp, "rocprim::inclusive_scan", [&](void *t, size_t &tb) { return rocprim::inclusive_scan(t, tb, in, out + 1, (size_t)n, rocprim::plus<int32_t>(), st); }); });
		return get32(out + n);
	}
	template <class Op> uint64_t reduce(const char *nm, const uint64_t *in, int64_t n, Op op)
	{
		if (n <= 0) return 0;
		if (!red_.p) red_.alloc(8);
		booked(nm, [&]() { dev_two_pass(tmp, "rocprim::reduce", [&](void *t, size_t &tb) { return rocprim::reduce(t, tb, in, red_.as<uint64_t>(), (uint64_t)0, (size_t)n, op, st); }); });
		return dev_get(red_.as<uint64_t>(), st);
	}
	uint64_t max64(const uint64_t *in, int64_t n) { return reduce("fs_max", in, n, rocprim::maximum<uint64_t>()); }
	uint64_t or64(const uint64_t *in, int64_t n) { return reduce("fs_or", in, n, FsOr()); }
	int64_t get(const int64_t *p) { return dev_get(p, st); }
	int32_t get32(const int32_t *p) { return dev_get(p, st); }
	void fetch(void *host, const void *dev, size_t bytes)
	{
		ARX_HIP_CHECK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
		ARX_HIP_CHECK(hipStreamSynchronize(st));
	}
	void sort_pairs(const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, int64_t n, int bits) { booked("fs_sort", [&]() { dev_sort_pairs(tmp, kin, kout, vin, vout, (size_t)n, bits, st); }); }
	void *work(int slot, int64_t bytes)
	{
		DevBuf &b = work_[slot];
		if (!b.p || (size_t)bytes > b.bytes) {
			ARX_HIP_CHECK(hipStreamSynchronize(st)); // what still reads the old buffer has ended
			b.alloc((size_t)bytes + (size_t)bytes / 4);
		}
		return b.p;
	}
	FsRec *table(int64_t n)
	{
		if (n > tab_n_) {
			const int64_t room = fs_table_room(n);
			DevBuf t((size_t)room * sizeof(FsRec));
			if (tab_n_) ARX_HIP_CHECK(hipMemcpyAsync(t.p, tab_.p, (size_t)tab_n_ * sizeof(FsRec), hipMemcpyDeviceToDevice, st));
			ARX_HIP_CHECK(hipStreamSynchronize(st));
			tab_ = std::move(t); tab_n_ = room;
		}
		return tab_.as<FsRec>();
	}
};

// ---- where the slabs go.  Two pairs of device buffers: the gather of slab k runs while slab k - 1 is consumed (its gather is awaited through an event)
struct FsSink {
	hipStream_t st = nullptr; // the gather's stream
	Stream out;               // the fetches' stream
	Event done[2];
	DevBuf buf[2][2];
	bool have = false;
	int64_t pk = 0, pb[2] = {0, 0};
	double us_consume = 0;
	virtual ~FsSink() {}
	void init(hipStream_t gather_stream)
	{
		st = gather_stream;
		out.create();
		for (Event &e : done) e.create(hipEventDisableTiming);
	}
	void take(int64_t k, int64_t cap, int64_t, int64_t, uint8_t **d1, uint8_t **d2)
	{
		for (int f = 0; f < 2; ++f)
			if (!buf[k & 1][f].p || (size_t)cap > buf[k & 1][f].bytes) buf[k & 1][f].alloc((size_t)cap);
		*d1 = buf[k & 1][0].as<uint8_t>(); *d2 = buf[k & 1][1].as<uint8_t>();
	}
	void give(int64_t k, int64_t, int64_t, int64_t b1, int64_t b2)
	{
		ARX_HIP_CHECK(hipEventRecord(done[k & 1], st));
		flush();
		have = true; pk = k; pb[0] = b1; pb[1] = b2;
	}
	void flush()
	{
		if (!have) return;
		have = false;
		ARX_HIP_CHECK(hipEventSynchronize(done[pk & 1]));
		const double t0 = bs_now_us();
		for (int f = 0; f < 2; ++f) consume(f, buf[pk & 1][f].as<uint8_t>(), pb[f]);
		us_consume += bs_now_us() - t0;
	}
	// n bytes of file f's output, complete in device memory; returns when they may be overwritten
	virtual void consume(int f, const uint8_t *d, int64_t n) = 0;
	void fetch(void *host, const uint8_t *d, int64_t n)
	{
		ARX_HIP_CHECK(hipMemcpyAsync(host, d, (size_t)n, hipMemcpyDeviceToHost, out));
		ARX_HIP_CHECK(hipStreamSynchronize(out));
	}
};
struct FsMemSink : FsSink { // the self-test's: into host memory
	std::vector<uint8_t> text[2];
	void consume(int f, const uint8_t *d, int64_t n) override
	{
		const size_t at = text[f].size();
		text[f].resize(at + (size_t)n);
		if (n) fetch(text[f].data() + at, d, n);
	}
};

// an output file: written as <path>.tmp, renamed by commit(), removed where that was not reached
struct FsOutFile {
	FILE *f = nullptr;
	std::string path, tmp; // tmp: empty unless this call created it -- nothing else is ever removed
	int64_t bytes_out = 0;
	bool open(const char *p)
	{
		path = p; tmp = path + ".tmp";
		f = fopen(tmp.c_str(), "wb");
		if (f) setvbuf(f, nullptr, _IOFBF, 1 << 20);
		else tmp.clear();
		return f != nullptr;
	}
	bool commit()
	{
		bool ok = f && fflush(f) == 0 && !ferror(f);
		if (f) { ok = fclose(f) == 0 && ok; f = nullptr; }
		ok = ok && rename(tmp.c_str(), path.c_str()) == 0;
		if (ok) tmp.clear();
		return ok;
	}
	~FsOutFile()
	{
		if (f) fclose(f);
		if (!tmp.empty()) remove(tmp.c_str());
	}
};
struct FsFileSink : FsSink {
	FsOutFile file[2];
	bool bgzf = false;
	std::shared_ptr<DeviceBgzf> z;
	std::vector<uint8_t> carry[2]; // BGZF: the bytes short of a block
	PinnedBuf h;
	double us_compress = 0, us_write = 0;
	void open(const char *const out_path[2]) // both <out>.tmp
	{
		for (int f = 0; f < 2; ++f)
			if (!file[f].open(out_path[f])) throw FsIoError(std::string("cannot write ") + out_path[f] + ".tmp");
	}
	// get_z: the device's compressor (arx_bgzf.hip keeps one per device)
	void begin(hipStream_t gather_stream, int device, std::shared_ptr<DeviceBgzf> (*get_z)(int))
	{
		init(gather_stream);
		if (bgzf) z = get_z(device);
	}
	void consume(int f, const uint8_t *d, int64_t n) override
	{
		if (n <= 0) return;
		const double t0 = bs_now_us();
		if (bgzf) {
			std::vector<uint8_t> tail;
			size_t nb = 0;
			std::string err;
			if (!z->run_device(carry[f].data(), carry[f].size(), d, (size_t)n, file[f].f, file[f].bytes_out, nb, tail, err)) throw FsIoError(file[f].path + ": " + err);
			carry[f].swap(tail);
			us_compress += bs_now_us() - t0;
			return;
		}
		if (!h.p || (size_t)n > h.bytes) h.alloc((size_t)n);
		fetch(h.p, d, n);
		if (fwrite(h.p, 1, (size_t)n, file[f].f) != (size_t)n) throw FsIoError(file[f].path + ": write failed");
		file[f].bytes_out += n;
		us_write += bs_now_us() - t0;
	}
	// the last block and the EOF block of a BGZF output; both files to their names
	void finish()
	{
		flush();
		const double t0 = bs_now_us();
		for (int f = 0; f < 2; ++f) {
			if (bgzf) {
				static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
				std::string err;
				if (!carry[f].empty() && !z->run(carry[f].data(), carry[f].size(), file[f].f, file[f].bytes_out, err, nullptr)) throw FsIoError(file[f].path + ": " + err);
				carry[f].clear();
				if (fwrite(eof, 1, 28, file[f].f) != 28) throw FsIoError(file[f].path + ": write failed");
				file[f].bytes_out += 28;
			}
		}
		for (int f = 0; f < 2; ++f)
			if (!file[f].commit()) throw FsIoError(file[f].path + ": write failed");
		us_write += bs_now_us() - t0;
	}
	template <class Drv> void end(Drv &drv) // finish(), its times booked
	{
		finish();
		drv.us[FS_T_COMPRESS] = us_compress; drv.us[FS_T_WRITE] = us_write;
	}
};

inline void fs_stats(int64_t *stats, const FsHipDrv &drv, const FsCounts &c, int64_t n1, int64_t n2, bool written)
{
	if (!stats) return;
	stats[0] = c.n_records; stats[1] = n1; stats[2] = n2; stats[3] = written ? c.bytes1 : 0; stats[4] = written ? c.bytes2 : 0; stats[5] = c.skipped; stats[6] = c.runs_in; stats[7] = c.distinct;
	stats[8] = c.max_bc; stats[9] = c.passes; stats[10] = c.windows; stats[11] = written ? c.slabs : 0;
	for (int k = FS_T_READ; k < FS_N_STATS; ++k) stats[k] = (int64_t)drv.us[k];
}

// table, order and (sink != null) gather of two texts in device memory.  rows: what the records are to the sort (dev_fqmerge.h: FxPlainRows;
// dev_fqprep.h: FpRows, which composes the key and the header).  Without `timed` the phases are wall-clock times between their ends: keys and
// sort passes together under FS_T_SORT; with it every launch group is awaited and booked on its own
template <class Rows> void fs_run_by(FsHipDrv &drv, const FsText &T, int64_t window, int64_t slab, FsSink *sink, FsCounts &c, FsSortMem &m, Rows &rows)
{
	double t0 = bs_now_us();
	const int rc = fs_parse(drv, T, window, c);
	if (rc == FS_E_RECORDS) throw FsTooLarge(std::string("more than 2^32 - 1 records") + FS_REMEDY);
	if (rc != FS_OK) throw FsTooLarge("a line or a record is longer than the " + std::to_string(window) + " bytes of a parse window");
	ARX_HIP_CHECK(hipStreamSynchronize(drv.st));
	if (!drv.timed) drv.us[FS_T_PARSE] = bs_now_us() - t0;
	t0 = bs_now_us();
	for (int s = FS_W_WIN1; s < FS_W_KEYS0; ++s) drv.work_[s].release(); // the parse's buffers make room for the sort's
	const int64_t N = c.n_records;
	fs_sort_mem(drv, N, m);
	const auto key = rows.key(drv, T, drv.tab_.as<FsRec>(), N, m);
	const int64_t longest = fs_order_by(drv, key, N, m, c);
	ARX_HIP_CHECK(hipStreamSynchronize(drv.st));
	if (!drv.timed) drv.us[FS_T_SORT] = bs_now_us() - t0;
	c.slabs = 0;
	if (!sink) return;
	t0 = bs_now_us();
	rows.gather(drv, T, key, N, m, slab, longest, *sink, c);
	sink->flush();
	if (!drv.timed) drv.us[FS_T_GATHER] = bs_now_us() - t0 - sink->us_consume;
}
inline void fs_run(FsHipDrv &drv, const FsText &T, int64_t window, int64_t slab, FsSink *sink, FsCounts &c, FsSortMem &m)
{
	FxPlainRows rows;
	fs_run_by(drv, T, window, slab, sink, c, m, rows);
}

// ---- the way in.  One input file: its reader, and (where a call holds the whole text) its text in device memory
// a gzip input that the device inflates: the reader thread's raw slabs as the compressed bytes of gunzip_host.h's reader
struct FsGzSlabs : GzSource {
	SlabReader *rd = nullptr;
	const SlabReader::Slab *s = nullptr;
	size_t at = 0;
	bool err = false, ended = false;
	size_t read(uint8_t *to, size_t n) override
	{
		size_t got = 0;
		while (got < n && !ended) {
			if (!s) {
				s = rd->acquire();
				at = 0;
				if (!s || s->err) { err = s != nullptr; ended = true; break; }
			}
			const size_t k = n - got < s->len - at ? n - got : s->len - at;
			if (k) memcpy(to + got, s->buf + at, k);
			at += k; got += k;
			if (at == s->len) {
				if (s->eof) ended = true;
				rd->release();
				s = nullptr;
			}
		}
		return got;
	}
};
// What the gzip inputs of the file calls did on the device, summed over the process: a file call's own statistics have no room for it, and a
// caller (or a test) must be able to see that the device took a file and why the host took over where it did.  arx_fastq_gunzip_counters
enum { GZC_FILES = 0, GZC_LAUNCHES, GZC_ACCEPTED, GZC_BYTES, GZC_HOST_BYTES, GZC_FALLBACK /* + the reason, 1 .. 6 */, GZC_N = GZC_FALLBACK + 7 };
inline std::atomic<int64_t> *gz_counters()
{
	static std::atomic<int64_t> c[GZC_N];
	return c;
}
struct FsGunzip {
	~FsGunzip() // however the reading ended
	{
		if (!rd) return;
		std::atomic<int64_t> *c = gz_counters();
		++c[GZC_FILES];
		c[GZC_LAUNCHES] += rd->stats[GZS_LAUNCHES]; c[GZC_ACCEPTED] += rd->stats[GZS_ACCEPTED]; c[GZC_BYTES] += rd->delivered; c[GZC_HOST_BYTES] += rd->stats[GZS_HOST_BYTES];
		const int64_t why = rd->stats[GZS_REASON];
		if (why > 0 && why <= 6) ++c[GZC_FALLBACK + why];
	}
	GzHip dev;
	FsGzSlabs src;
	std::unique_ptr<GzReader<GzHip> > rd;
	void begin(hipStream_t st, SlabReader *slabs)
	{
		dev.init(st);
		src.rd = slabs;
		const int64_t cap = (int64_t)slabs->slab_cap(), slab = cap < GZ_SLAB_DEFAULT ? (cap < 2 * GZ_CHUNK_DEFAULT ? 2 * GZ_CHUNK_DEFAULT : cap) : GZ_SLAB_DEFAULT;
		rd.reset(new GzReader<GzHip>(dev, src, GZ_CHUNK_DEFAULT, slab, GZ_EXPAND_DEFAULT));
	}
};

struct FsInput {
	std::unique_ptr<SlabReader> rd;
	bool bgzf = false, gunzip = false, done = false;
	std::unique_ptr<FsGunzip> gz; // made by the first take(): the device is chosen by then
	DevBuf text;
	int64_t len = 0;
	template <class R> bool open_as(const char *path, size_t chunk)
	{
		std::unique_ptr<R> r(new R());
		const bool ok = r->open(path, chunk, FS_READ_CHUNKS);
		rd = std::move(r);
		return ok;
	}
	bool open(const char *path, size_t chunk = FS_READ_CHUNK, bool gunzip_device = false)
	{
		bgzf = file_is_bgzf(path);
		gunzip = gunzip_device && !bgzf && file_is_gzip(path);
		return bgzf ? open_as<BgzfChunkReader>(path, chunk) : gunzip ? open_as<GzipRawReader>(path, chunk) : open_as<ChunkReader>(path, chunk);
	}
	void room(int64_t need, hipStream_t st) // the text so far stays
	{
		if (text.p && (size_t)need <= text.bytes) return;
		DevBuf t((size_t)(need + need / 2) + 64);
		if (len) ARX_HIP_CHECK(hipMemcpyAsync(t.p, text.p, (size_t)len, hipMemcpyDeviceToDevice, st));
		ARX_HIP_CHECK(hipStreamSynchronize(st));
		text = std::move(t);
	}
};
inline void fs_open_inputs(FsInput in[2], const char *const path[2], size_t chunk = FS_READ_CHUNK, bool gunzip_device = false)
{
	for (int f = 0; f < 2; ++f)
		if (!in[f].open(path[f], chunk, gunzip_device)) throw FsIoError(std::string("cannot read ") + path[f]);
}
// for the calls that touch the device before they open their readers: a missing input is refused first
inline void fs_probe_inputs(const char *const path[2])
{
	for (int f = 0; f < 2; ++f) {
		FILE *p = fopen(path[f], "rb");
		if (!p) throw FsIoError(std::string("cannot read ") + path[f]);
		fclose(p);
	}
}

// a reader's slab to dst in device memory: plain text goes up as it is, of a BGZF slab only the compressed bytes go up and are inflated there
struct FsSlabUp {
	DevBuf d_comp, d_rows, d_status;
	void run(hipStream_t st, const SlabReader::Slab &s, bool bgzf, uint8_t *dst, const char *path)
	{
		if (!bgzf) {
			if (s.len) ARX_HIP_CHECK(hipMemcpyAsync(dst, s.buf, s.len, hipMemcpyHostToDevice, st));
		} else if (s.n_rows) {
			const size_t nr = s.n_rows;
			if (!d_comp.p || s.len > d_comp.bytes) d_comp.alloc(s.len + s.len / 4);
			if (!d_rows.p || nr * sizeof(InfRow) > d_rows.bytes) { d_rows.alloc(2 * nr * sizeof(InfRow)); d_status.alloc(4 * (2 * nr + 2)); }
			ARX_HIP_CHECK(hipMemcpyAsync(d_comp.p, s.buf, s.len, hipMemcpyHostToDevice, st));
			ARX_HIP_CHECK(hipMemcpyAsync(d_rows.p, s.rows, nr * sizeof(InfRow), hipMemcpyHostToDevice, st));
			ARX_HIP_CHECK(hipMemsetAsync(d_status.p, 0, 4 * (nr + 2), st));
			int32_t *counts = d_status.as<int32_t>() + nr;
			inflate_launch(st, d_comp.as<uint8_t>(), (int64_t)s.len, d_rows.as<InfRow>(), (int)nr, dst, (int64_t)s.text, d_status.as<int32_t>(), counts);
			int32_t bad[2] = {0, 0};
			ARX_HIP_CHECK(hipMemcpyAsync(bad, counts, 8, hipMemcpyDeviceToHost, st));
			ARX_HIP_CHECK(hipStreamSynchronize(st));
			if (bad[0] != 0) throw FsIoError(std::string(path) + ": a BGZF block does not inflate");
		}
		ARX_HIP_CHECK(hipStreamSynchronize(st)); // the reader may refill the slab
	}
	void release() { d_comp.release(); d_rows.release(); d_status.release(); }
};

// ---- the external sort (dev_fqmerge.h): arx_fastq_sort_ex with run_bytes != 0, arx_selftest_fastq_sort_ext
struct FxHipDrv : FsHipDrv {
	DevBuf run_[2], keep_[2];
	void *run_buf(int f, int64_t bytes) { run_[f].alloc((size_t)bytes); return run_[f].p; }
	void copy(void *dst, const void *src, int64_t n) { if (n > 0) ARX_HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)n, hipMemcpyDeviceToDevice, st)); }
	void upload(void *dev, const void *host, size_t bytes)
	{
		if (!bytes) return;
		ARX_HIP_CHECK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st));
		ARX_HIP_CHECK(hipStreamSynchronize(st));
	}
	void *keep(int which, int64_t bytes, int64_t kept) // grows by half, as the table
	{
		DevBuf &b = keep_[which];
		if (!b.p || (size_t)bytes > b.bytes) {
			DevBuf t((size_t)(bytes + bytes / 2));
			if (kept) ARX_HIP_CHECK(hipMemcpyAsync(t.p, b.p, (size_t)kept, hipMemcpyDeviceToDevice, st));
			ARX_HIP_CHECK(hipStreamSynchronize(st));
			b = std::move(t);
		}
		return b.p;
	}
	void runs_done() // what only the runs needed makes room for the merge's order
	{
		ARX_HIP_CHECK(hipStreamSynchronize(st));
		for (DevBuf &b : run_) b.release();
		for (DevBuf &b : work_) b.release();
		tab_.release(); tab_n_ = 0;
	}
};

// where the sorted runs wait for the merge: one store per sort, the runs of file f appended one after another to its one file
struct FxRunStore {
	int64_t bytes[2] = {0, 0};
	virtual ~FxRunStore() {}
	virtual void append(int f, const void *p, int64_t n) = 0;
	virtual void read(int f, int64_t at, int64_t n, void *dst) = 0;
};
struct FxMemStore : FxRunStore { // the self-test's
	std::vector<uint8_t> text[2];
	void append(int f, const void *p, int64_t n) override { text[f].insert(text[f].end(), (const uint8_t *)p, (const uint8_t *)p + n); bytes[f] += n; }
	void read(int f, int64_t at, int64_t n, void *dst) override
	{
		if (at < 0 || n < 0 || at + n > bytes[f]) throw FsIoError("a range outside the sorted runs");
		memcpy(dst, text[f].data() + at, (size_t)n);
	}
};
// a temporary file under a name of its own (mkstemps), removed when its owner goes
struct FxTmpFile {
	int fd = -1;
	std::string path;
	bool create(const std::string &dir, const char *suffix)
	{
		std::string t = dir + "/arx_fqsort_XXXXXX" + suffix;
		fd = mkstemps(&t[0], (int)strlen(suffix));
		if (fd >= 0) path = t;
		return fd >= 0;
	}
	~FxTmpFile()
	{
		if (fd >= 0) close(fd);
		if (!path.empty()) unlink(path.c_str());
	}
};
struct FxFileStore : FxRunStore {
	FxTmpFile file[2];
	void create(const char *tmp_dir, const char *out1) // both run files, under tmp_dir or (null) in the directory of the first output
	{
		std::string dir = tmp_dir ? tmp_dir : out1;
		if (!tmp_dir) { const size_t cut = dir.rfind('/'); dir = cut == std::string::npos ? "." : cut == 0 ? "/" : dir.substr(0, cut); }
		for (int f = 0; f < 2; ++f)
			if (!file[f].create(dir, f ? ".r2" : ".r1")) throw FsIoError("cannot write a temporary file under " + dir);
	}
	void append(int f, const void *p, int64_t n) override
	{
		for (int64_t done = 0; done < n;) {
			const ssize_t k = pwrite(file[f].fd, (const char *)p + done, (size_t)(n - done), (off_t)(bytes[f] + done));
			if (k <= 0) throw FsIoError(file[f].path + ": write failed");
			done += k;
		}
		bytes[f] += n;
	}
	void read(int f, int64_t at, int64_t n, void *dst) override
	{
		for (int64_t done = 0; done < n;) {
			const ssize_t k = pread(file[f].fd, (char *)dst + done, (size_t)(n - done), (off_t)(at + done));
			if (k <= 0) throw FsIoError(file[f].path + ": read failed");
			done += k;
		}
	}
};

// dev_fqmerge.h's io: a run's slabs to the store (a sink of fs_gather), and the store's ranges to the merge's stage buffers through page-locked memory
struct FxIo : FsSink {
	FxRunStore *store = nullptr;
	PinnedBuf h, hs;
	struct Up { void *dst; size_t at, n; };
	std::vector<Up> ups;
	size_t used = 0;
	double us_write = 0, us_read = 0;
	void consume(int f, const uint8_t *d, int64_t n) override
	{
		if (n <= 0) return;
		const double t0 = bs_now_us();
		if (!h.p || (size_t)n > h.bytes) h.alloc((size_t)n);
		fetch(h.p, d, n);
		store->append(f, h.p, n);
		us_write += bs_now_us() - t0;
	}
	void end_run() { flush(); }
	void runs_done() // the merge's sink has slab buffers of its own
	{
		for (auto &pair : buf) for (DevBuf &b : pair) b.release();
		h.release();
	}
	void begin(int64_t bytes)
	{
		if (!hs.p || (size_t)bytes > hs.bytes) hs.alloc((size_t)bytes);
		used = 0; ups.clear();
	}
	void read(int f, int64_t at, int64_t n, uint8_t *dst)
	{
		const double t0 = bs_now_us();
		store->read(f, at, n, hs.as<uint8_t>() + used);
		ups.push_back(Up{dst, used, (size_t)n});
		used += (size_t)n;
		us_read += bs_now_us() - t0;
	}
	void staged()
	{
		const double t0 = bs_now_us();
		for (const Up &u : ups) ARX_HIP_CHECK(hipMemcpyAsync(u.dst, hs.as<uint8_t>() + u.at, u.n, hipMemcpyHostToDevice, st));
		ARX_HIP_CHECK(hipStreamSynchronize(st)); // hs may be refilled
		us_read += bs_now_us() - t0;
	}
};

constexpr int FX_N_STATS = 24;
enum { FX_RUNS = 20, FX_TMP_BYTES, FX_T_RUN_WRITE, FX_T_RUN_READ };
constexpr int64_t FX_AUTO_RESERVE = (int64_t)1 << 30, FX_AUTO_SHARE = 8, FX_AUTO_MOST = (int64_t)16 << 30;

// run_bytes == -1: an eighth of the free device memory less 1 GiB, in whole MiB, 16 GiB at most (include/arachne_amd.h has the accounting)
inline int64_t fx_auto_run_bytes(int64_t least, int64_t share = FX_AUTO_SHARE)
{
	size_t fr = 0, total = 0;
	ARX_HIP_CHECK(hipMemGetInfo(&fr, &total));
	int64_t rb = ((int64_t)fr - FX_AUTO_RESERVE) / share;
	rb &= ~(((int64_t)1 << 20) - 1);
	if (rb > FX_AUTO_MOST) rb = FX_AUTO_MOST;
	return rb < least ? least : rb;
}

// runs, merge and (sink != null) output of what src delivers; store == null: CHECK, only the keys are kept.  rows: what a run's records are
// to the sort (dev_fqmerge.h: FxPlainRows; dev_fqprep.h: FpRows)
template <class Src, class Rows> void fx_run_by(FxHipDrv &drv, Src &src, FxRunStore *store, FsSink *sink, int64_t run_bytes, int64_t window, int64_t slab, FsCounts &c, FsSortMem &m, FxRuns &S, FxIo &io,
                                                Rows &rows)
{
	double t0 = bs_now_us();
	io.store = store;
	if (store) io.init(drv.st);
	const double fed0 = drv.us[FS_T_READ] + drv.us[FS_T_INFLATE];
	const int rc = fx_runs_by(drv, src, store ? &io : nullptr, run_bytes, window, slab, S, rows);
	if (rc == FS_E_RECORDS) throw FsTooLarge(std::string("more than 2^32 - 1 records") + FS_REMEDY);
	if (rc == FS_E_TOO_LARGE) throw FsTooLarge("a line or a record is longer than the " + std::to_string(window) + " bytes of a parse window");
	if (rc == FS_E_RUN) throw FsTooLarge("a line or a record does not fit a run of " + std::to_string(run_bytes) + " bytes per file: use a larger run_bytes");
	if (rc == FS_E_RUNS) throw FsTooLarge("more than " + std::to_string(FS_MAX_RUNS) + " sorted runs of " + std::to_string(run_bytes) + " bytes per file: use a larger run_bytes");
	if (rc != FS_OK) throw std::runtime_error("the external sort failed in its runs");
	drv.runs_done();
	io.runs_done();
	if (!drv.timed) drv.us[FS_T_SORT] = bs_now_us() - t0 - io.us_write - (drv.us[FS_T_READ] + drv.us[FS_T_INFLATE] - fed0);
	t0 = bs_now_us();
	if (fx_merge(drv, &io, sink, S, slab, m, c) != FS_OK) throw std::runtime_error("the external sort's merge: the staged ranges are not the slab's bytes");
	if (sink) sink->flush();
	ARX_HIP_CHECK(hipStreamSynchronize(drv.st));
	if (!drv.timed) drv.us[FS_T_GATHER] = bs_now_us() - t0 - io.us_read - (sink ? sink->us_consume : 0);
}
template <class Src> void fx_run(FxHipDrv &drv, Src &src, FxRunStore *store, FsSink *sink, int64_t run_bytes, int64_t window, int64_t slab, FsCounts &c, FsSortMem &m, FxRuns &S, FxIo &io)
{
	FxPlainRows rows;
	fx_run_by(drv, src, store, sink, run_bytes, window, slab, c, m, S, io, rows);
}
inline void fx_stats(int64_t *stats, const FxHipDrv &drv, const FsCounts &c, int64_t n1, int64_t n2, bool written, const FxRuns &S, const FxIo &io)
{
	if (!stats) return;
	fs_stats(stats, drv, c, n1, n2, written);
	stats[FX_RUNS] = S.n_runs; stats[FX_TMP_BYTES] = written ? S.file1 + S.file2 : 0;
	stats[FX_T_RUN_WRITE] = (int64_t)io.us_write; stats[FX_T_RUN_READ] = (int64_t)io.us_read;
}

// two texts in host memory (the self-test's source)
struct FxMemSrc {
	hipStream_t st;
	const uint8_t *t[2];
	int64_t n[2], at[2] = {0, 0};
	FxMemSrc(hipStream_t s, const uint8_t *t1, int64_t n1, const uint8_t *t2, int64_t n2) : st(s), t{t1, t2}, n{n1, n2} {}
	bool ended(int f) const { return at[f] == n[f]; }
	int64_t fill(int f, uint8_t *dst, int64_t want)
	{
		const int64_t k = want < n[f] - at[f] ? want : n[f] - at[f];
		if (k > 0) {
			ARX_HIP_CHECK(hipMemcpyAsync(dst, t[f] + at[f], (size_t)k, hipMemcpyHostToDevice, st));
			ARX_HIP_CHECK(hipStreamSynchronize(st));
		}
		at[f] += k;
		return k;
	}
};
// the two files through their readers.  A reader's slab goes up (and, BGZF, is inflated: FsSlabUp) either into a buffer of its own -- the runs
// and the windows take their bytes from there, so a slab that straddles a run's end is split and its rest opens the next run -- or, for a call
// that holds both whole texts, straight to its place in them (load)
struct FxFileSrc {
	FsInput *in = nullptr;        // [2]
	const char *const *path = nullptr;
	FsHipDrv *drv = nullptr;
	int64_t max_bytes = 0;
	const char *remedy = "";      // the end of the max_bytes refusal, which is the call's own
	DevBuf text[2];
	FsSlabUp up;
	int64_t have[2] = {0, 0}, at[2] = {0, 0}, total[2] = {0, 0};
	void start(FsInput *inputs, const char *const *paths, FsHipDrv &d, int64_t most = 0, const char *most_remedy = "")
	{
		in = inputs; path = paths; drv = &d; max_bytes = most; remedy = most_remedy;
		for (int f = 0; f < 2; ++f) in[f].rd->start();
	}
	bool ended(int f) const { return in[f].done && at[f] == have[f]; }
	// the next slab of file f to dst(its bytes of text) -> those bytes; -1: the file has ended
	template <class Dst> int64_t take(int f, Dst dst)
	{
		FsInput &I = in[f];
		if (I.gunzip) return take_gunzip(f, dst);
		double t0 = bs_now_us();
		const SlabReader::Slab *s = I.rd->acquire();
		drv->us[FS_T_READ] += bs_now_us() - t0;
		if (!s) { I.done = true; return -1; }
		t0 = bs_now_us();
		if (s->err) throw FsIoError(std::string(path[f]) + (I.bgzf ? ": not a chain of whole BGZF blocks" : ": read error"));
		if (max_bytes > 0 && total[0] + total[1] + (int64_t)s->text > max_bytes)
			throw FsTooLarge(std::string(path[0]) + " and " + path[1] + " inflate to more than the " + std::to_string(max_bytes) + " bytes allowed" + remedy);
		const int64_t n = (int64_t)s->text;
		up.run(drv->st, *s, I.bgzf, dst(n), path[f]);
		total[f] += n;
		if (s->eof) I.done = true;
		I.rd->release();
		drv->us[FS_T_INFLATE] += bs_now_us() - t0;
		return n;
	}
	// the same of a gzip file that the device inflates: the next piece's size first, then its place, then the resolve straight into it
	template <class Dst> int64_t take_gunzip(int f, Dst dst)
	{
		FsInput &I = in[f];
		const double t0 = bs_now_us();
		if (!I.gz) { I.gz.reset(new FsGunzip()); I.gz->begin(drv->st, I.rd.get()); }
		const int64_t n = I.gz->rd->next();
		if (n == GZ_ERROR || I.gz->src.err) throw FsIoError(std::string(path[f]) + ": read error");
		if (n == GZ_END) { I.done = true; return -1; }
		if (max_bytes > 0 && total[0] + total[1] + n > max_bytes)
			throw FsTooLarge(std::string(path[0]) + " and " + path[1] + " inflate to more than the " + std::to_string(max_bytes) + " bytes allowed" + remedy);
		I.gz->rd->place(dst(n));
		total[f] += n;
		drv->us[FS_T_INFLATE] += bs_now_us() - t0;
		return n;
	}
	void next(int f) // the next slab of file f into text[f]
	{
		have[f] = at[f] = 0;
		const int64_t n = take(f, [&](int64_t bytes) {
			if (!text[f].p || (size_t)bytes > text[f].bytes) { ARX_HIP_CHECK(hipStreamSynchronize(drv->st)); text[f].alloc((size_t)bytes + 64); }
			return text[f].as<uint8_t>();
		});
		if (n > 0) have[f] = n;
	}
	int64_t fill(int f, uint8_t *dst, int64_t want)
	{
		int64_t got = 0;
		while (got < want && !ended(f)) {
			if (at[f] == have[f]) { next(f); continue; }
			const int64_t k = want - got < have[f] - at[f] ? want - got : have[f] - at[f];
			ARX_HIP_CHECK(hipMemcpyAsync(dst + got, text[f].as<uint8_t>() + at[f], (size_t)k, hipMemcpyDeviceToDevice, drv->st));
			at[f] += k; got += k;
		}
		while (at[f] == have[f] && !in[f].done) next(f); // so that ended() knows of an end that lies right here
		return got;
	}
	// both whole texts into device memory (in[f].text), slab by slab as the readers have them, every slab inflated straight to its place; the
	// readers and the slab buffers are gone afterwards
	FsText load()
	{
		while (!in[0].done || !in[1].done)
			for (int f = 0; f < 2; ++f) {
				FsInput &I = in[f];
				if (I.done) continue;
				const int64_t n = take(f, [&](int64_t bytes) { I.room(I.len + bytes, drv->st); return I.text.as<uint8_t>() + I.len; });
				if (n > 0) I.len += n;
			}
		for (int f = 0; f < 2; ++f) { in[f].gz.reset(); in[f].rd.reset(); text[f].release(); }
		up.release();
		return FsText{in[0].text.as<uint8_t>(), in[1].text.as<uint8_t>(), in[0].len, in[1].len};
	}
};

// arx_fastq_sort.  What is refused is thrown: FsIoError, FsTooLarge
inline void fs_sort_files(int device, const char *const in_path[2], const char *const out_path[2], int flags, int64_t max_bytes, int64_t *stats, std::shared_ptr<DeviceBgzf> (*get_z)(int))
{
	const bool check = (flags & ARX_FQSORT_CHECK) != 0;
	FsInput in[2];
	fs_open_inputs(in, in_path, FS_READ_CHUNK, (flags & ARX_FQSORT_GUNZIP_DEVICE) != 0);
	FsFileSink sink;
	sink.bgzf = (flags & ARX_FQSORT_BGZF) != 0;
	if (!check) sink.open(out_path);
	select_device(device, FS_NO_DEVICE);
	Stream st; // the call's own; declared before the buffers, so that it has ended when they are freed
	st.create();
	FsHipDrv drv; drv.st = st; drv.timed = (flags & ARX_FQSORT_TIMED) != 0;
	FxFileSrc src;
	src.start(in, in_path, drv, max_bytes, FS_REMEDY);
	const FsText T = src.load();
	FsCounts c{};
	FsSortMem m{};
	if (!check) sink.begin(st, device, get_z);
	fs_run(drv, T, FS_WINDOW_DEFAULT, FS_SLAB_DEFAULT, check ? nullptr : &sink, c, m);
	if (!check) sink.end(drv);
	fs_stats(stats, drv, c, T.n1, T.n2, !check);
}

// arx_fastq_sort_ex with run_bytes != 0
inline void fx_sort_files(int device, const char *const in_path[2], const char *const out_path[2], int flags, int64_t max_bytes, int64_t run_bytes, const char *tmp_dir, int64_t *stats,
                          std::shared_ptr<DeviceBgzf> (*get_z)(int))
{
	const bool check = (flags & ARX_FQSORT_CHECK) != 0;
	FsInput in[2];
	fs_open_inputs(in, in_path, FS_READ_CHUNK, (flags & ARX_FQSORT_GUNZIP_DEVICE) != 0);
	FsFileSink sink;
	sink.bgzf = (flags & ARX_FQSORT_BGZF) != 0;
	FxFileStore store;
	if (!check) {
		sink.open(out_path);
		store.create(tmp_dir, out_path[0]);
	}
	select_device(device, FS_NO_DEVICE);
	Stream st; // the call's own; declared before the buffers, so that it has ended when they are freed
	st.create();
	FxHipDrv drv; drv.st = st; drv.timed = (flags & ARX_FQSORT_TIMED) != 0;
	const int64_t rb = run_bytes == -1 ? fx_auto_run_bytes(FS_WINDOW_DEFAULT) : run_bytes;
	FsCounts c{};
	FsSortMem m{};
	FxRuns S;
	FxIo io;
	FxFileSrc src;
	src.start(in, in_path, drv, max_bytes);
	if (!check) sink.begin(st, device, get_z);
	fx_run(drv, src, check ? nullptr : &store, check ? nullptr : &sink, rb, rb < FS_WINDOW_DEFAULT ? rb : FS_WINDOW_DEFAULT, FS_SLAB_DEFAULT, c, m, S, io);
	for (int f = 0; f < 2; ++f) { in[f].gz.reset(); in[f].rd.reset(); }
	if (!check) sink.end(drv);
	fx_stats(stats, drv, c, src.total[0], src.total[1], !check, S, io);
}

} // namespace arx

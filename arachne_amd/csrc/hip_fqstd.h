// hip_fqstd.h -- dev_fqstd.h on the GPU, and the driver behind arx_fastq_standardize and arx_selftest_fastq_standardize (arx_bgzf.hip): the headers
// of a haplotagging, stLFR or TELLseq FASTQ file pair rewritten to `@<id>/1\tBX:Z:<barcode>\tVX:i:<0|1>`, the step in front of arx_fastq_sort
// (the intended behaviour of the reference's src/preprocess/standardize.go, which does not compile).
//
// Everything it runs on is the sort's (hip_fqsort.h): k_fs_items<F> starts one item of a functor per thread through hip_launch under the
// functor's name (fqs_match, fqs_fields, fqs_compose beside the feeder's fq_* and fs_window), FsHipDrv supplies scans, reductions and work
// buffers, FqsFiles (fs_open_inputs and an FxFileSrc) brings the files in slab by slab (a BGZF file inflated on the device by inflate_launch,
// anything else through zlib on a reader thread), FsFileSink (open / begin / end) takes the output slabs from two pairs of buffers -- slab k is
// fetched and written, or compressed (DeviceBgzf::run_device) and written, while slab k + 1 is composed -- into <out>.tmp, renamed at the end
// and removed otherwise.  fqs_detect_files and fqs_detect_mem are the detection of every call that has one, arx_fastq_prepare's included.
//
// The call streams.  Device memory of a call, whatever the files' sizes: four window buffers (FS_WINDOW_DEFAULT each: two per file, the carry
// moves from one to the other), the readers' slab text per file (32 MiB each), the line index of a window (about a window's size again), 88 bytes
// per record of a window (fields, sizes, offsets, counts), four output slab buffers (FS_SLAB_DEFAULT each), rocprim's scratch: about 0.7 GiB.
// Detection is a pass of its own over the head of the files -- through readers with small slabs and a window of FQS_DETECT_WINDOW, so that it
// inflates a few MiB and not two slabs per file; a record that this window does not hold sends it to the full window, so the result is the full
// window's --; the readers are opened again for the conversion.
#pragma once
#include <initializer_list>
#include "hip_fqsort.h"
#include "dev_fqstd.h"

namespace arx {

constexpr int FQS_N_STATS = 20;
constexpr int64_t FQS_DETECT_WINDOW = (int64_t)4 << 20; // what detection looks at first, per file
constexpr size_t FQS_DETECT_CHUNK = (size_t)1 << 20;    // its readers' chunk
constexpr const char *FQS_NO_DEVICE = "no such HIP device: the FASTQ header standardization runs on the GPU (there is no CPU fallback)";

// FsHipDrv with dev_fqstd.h's clock.  Without `timed` the phases are wall-clock times between drv.phase() calls: a parse ends with a fetch, so its
// time holds what was still running of the compose before it; with `timed` every launch group is awaited and booked on its own (FsHipDrv::booked)
struct FqsHipDrv : FsHipDrv {
	int cur = -1;
	double mark = 0, wall[3] = {0, 0, 0};
	void phase(int k)
	{
		if (timed) return;
		const double now = bs_now_us();
		if (cur >= 0) wall[cur] += now - mark;
		cur = k; mark = now;
	}
	void pass_done() // everything of a pass has ended
	{
		ARX_HIP_CHECK(hipStreamSynchronize(st));
		phase(FQS_P_FILL);
		cur = -1;
	}
};

inline void fqs_stats(int64_t *stats, const FqsHipDrv &drv, const FqsCounts &c, int format, int64_t decided, double us_consume, double us_compress, double us_write)
{
	if (!stats) return;
	stats[0] = c.n_records; stats[1] = c.in1; stats[2] = c.in2; stats[3] = c.bytes1; stats[4] = c.bytes2; stats[5] = c.skipped; stats[6] = format; stats[7] = decided;
	stats[8] = c.with_bc; stats[9] = c.valid; stats[10] = c.max_bc; stats[11] = c.windows; stats[12] = c.slabs;
	stats[13] = (int64_t)drv.us[FS_T_READ]; stats[14] = (int64_t)drv.us[FS_T_INFLATE];
	if (drv.timed) { stats[15] = (int64_t)drv.us[FS_T_PARSE]; stats[16] = (int64_t)drv.us[FS_T_KEYS]; stats[17] = (int64_t)drv.us[FS_T_GATHER]; }
	else {
		const double compose = drv.wall[FQS_P_COMPOSE] - us_consume;
		stats[15] = (int64_t)drv.wall[FQS_P_PARSE]; stats[16] = 0; stats[17] = (int64_t)(compose > 0 ? compose : 0);
	}
	stats[18] = (int64_t)us_compress; stats[19] = (int64_t)us_write;
}

inline void fqs_throw(int rc, int64_t window)
{
	if (rc == FS_E_TOO_LARGE) throw FsTooLarge("a line or a record is longer than the " + std::to_string(window) + " bytes of a parse window");
	if (rc != FS_OK) throw std::runtime_error("the header standardization failed in its stream");
}

// the two files through their readers, from their first bytes
struct FqsFiles {
	FsInput in[2];
	FxFileSrc src;
	void open(const char *const path[2], FsHipDrv &drv, size_t chunk = FS_READ_CHUNK, int64_t max_bytes = 0, bool gunzip_device = false)
	{
		fs_open_inputs(in, path, chunk, gunzip_device);
		src.start(in, path, drv, max_bytes);
	}
};

// the format of a file pair from its head: FQS_DETECT_WINDOW of each file first, through readers with small slabs, a whole window only where a
// record does not fit that.  Drv: FqsHipDrv, or one with an empty phase() whose pass_done() only waits
template <class Drv> void fqs_detect_files(Drv &drv, const char *const in_path[2], FqsCounts &d, bool gunzip_device = false)
{
	for (const int64_t window : {FQS_DETECT_WINDOW, FS_WINDOW_DEFAULT}) {
		FqsFiles files;
		files.open(in_path, drv, window == FQS_DETECT_WINDOW ? FQS_DETECT_CHUNK : FS_READ_CHUNK, 0, gunzip_device);
		d = FqsCounts();
		const int rc = fqs_detect(drv, files.src, window, d);
		drv.pass_done();
		if (rc == FS_E_TOO_LARGE && window != FS_WINDOW_DEFAULT) continue; // a record of the head does not fit the small window
		fqs_throw(rc, window);
		break;
	}
}
// the same of two texts in host memory (the self-tests')
template <class Drv> void fqs_detect_mem(Drv &drv, const uint8_t *t1, int64_t n1, const uint8_t *t2, int64_t n2, int64_t window, FqsCounts &d)
{
	FxMemSrc src(drv.st, t1, n1, t2, n2);
	const int rc = fqs_detect(drv, src, window, d);
	drv.pass_done();
	fqs_throw(rc, window);
}
inline std::string fqs_no_format() { return "no record of the first " + std::to_string(FQS_DETECT_RECORDS) + " names a format (standard, haplotagging, stLFR, TELLseq): pass the format"; }

// arx_fastq_standardize.  What is refused is thrown: FsIoError, FsTooLarge, FsBadArg
inline void fqs_files(int device, const char *const in_path[2], const char *const out_path[2], int format, int flags, int64_t *stats, std::shared_ptr<DeviceBgzf> (*get_z)(int))
{
	const bool detect_only = (flags & ARX_FQSTD_DETECT) != 0, gunzip_device = (flags & ARX_FQSTD_GUNZIP_DEVICE) != 0;
	fs_probe_inputs(in_path);
	select_device(device, FQS_NO_DEVICE);
	Stream st; // the call's own; declared before the buffers, so that it has ended when they are freed
	st.create();
	FqsHipDrv drv; drv.st = st; drv.timed = (flags & ARX_FQSTD_TIMED) != 0;
	int fmt = format;
	int64_t decided = -1;
	if (format == FQS_AUTO || detect_only) {
		FqsCounts d;
		fqs_detect_files(drv, in_path, d, gunzip_device);
		fmt = d.format; decided = d.decided;
		if (detect_only || fmt == FQS_STANDARD) {
			d.n_records = 0; // nothing was written
			fqs_stats(stats, drv, d, fmt, decided, 0, 0, 0);
			return;
		}
		if (fmt == FQS_UNKNOWN) {
			if (stats) { stats[6] = fmt; stats[7] = -1; }
			throw FsBadArg(fqs_no_format());
		}
	}
	FqsFiles files;
	files.open(in_path, drv, FS_READ_CHUNK, 0, gunzip_device);
	FsFileSink sink;
	sink.bgzf = (flags & ARX_FQSTD_BGZF) != 0;
	sink.open(out_path);
	sink.begin(st, device, get_z);
	FqsCounts c;
	const int rc = fqs_convert(drv, files.src, fmt, FS_WINDOW_DEFAULT, FS_SLAB_DEFAULT, sink, c);
	fqs_throw(rc, FS_WINDOW_DEFAULT);
	drv.phase(FQS_P_FILL); // the last blocks and the rename are the sink's own time
	sink.end(drv);
	drv.pass_done();
	fqs_stats(stats, drv, c, fmt, decided, sink.us_consume, sink.us_compress, sink.us_write);
}

} // namespace arx

// hip_fqprep.h -- dev_fqprep.h on the GPU, and the driver behind arx_fastq_prepare and arx_selftest_fastq_prepare (arx_bgzf.hip): a haplotagging,
// stLFR or TELLseq FASTQ file pair standardized and sorted by barcode in one call -- the bytes of arx_fastq_sort_ex after arx_fastq_standardize,
// without the files between them.
//
// Everything it runs on is the sort's and the standardization's (hip_fqsort.h, hip_fqstd.h): k_fs_items<F> starts one item of a functor per
// thread through hip_launch under the functor's name (fp_fields and fp_gather beside fq_*, fs_*, fx_* and fqs_match), FxHipDrv supplies scans,
// reductions, the key sort and the buffers, FqsFiles / FxFileSrc bring the files in slab by slab (a BGZF file inflated on the device), FsFileSink
// takes the output slabs (plain text or device BGZF), FxFileStore and FxIo hold the sorted runs.  Detection is fqs_detect_files: a pass over the
// head of the files through readers of their own, the files opened again for the work.
//
//   AUTO finds standard   the call is fs_sort_files / fx_sort_files on the inputs, stats[24 ..] added
//   run_bytes == 0        both raw texts into device memory (FxFileSrc::load, every slab inflated straight to its place), then fs_run_by with
//                         FpRows: fs_parse, FpFieldsF, the order by the composed key, FpGatherF into the sink
//   run_bytes != 0        fx_run_by with FpRows: the run buffers hold raw text, the run files standardized text; the merge is the sort's
//
// Device memory.  Per record 120 bytes where the sort has 80 (dev_fqprep.h: the 40 bytes of FpRec more); everything else is the sort's
// accounting (hip_fqsort.h), the texts being the raw ones, which are shorter than what is written by about 17 bytes less the dropped R2 header
// per record.  run_bytes == -1: a run needs its two buffers and 120 bytes per record -- 2.4 run_bytes at 100 bytes of text per record and file,
// 4.4 run_bytes in all where the sort needs 3.6 --, so a TENTH of the free memory less 1 GiB keeps the runs at the same share of it, a little
// under half, and leaves the rest to what grows with the whole input (40 bytes and the key per record, 40 more while the merge orders).
// Nobody has measured which run size is fastest.
#pragma once
#include "hip_fqstd.h"
#include "dev_fqprep.h"

namespace arx {

constexpr int FP_N_STATS = 28;
enum { FP_S_FORMAT = 24, FP_S_DECIDED, FP_S_WITH_BC, FP_S_VALID };
constexpr int64_t FP_AUTO_SHARE = 10;
constexpr const char *FP_NO_DEVICE = "no such HIP device: the FASTQ preparation runs on the GPU (there is no CPU fallback)";

struct FpHipDrv : FxHipDrv {
	void phase(int) {} // fqs_detect's clock: the detection is not booked
	void pass_done() { ARX_HIP_CHECK(hipStreamSynchronize(st)); }
};

inline void fp_stats(int64_t *stats, int format, int64_t decided, const FpRows &rows)
{
	if (!stats) return;
	stats[FP_S_FORMAT] = format; stats[FP_S_DECIDED] = decided; stats[FP_S_WITH_BC] = rows.with_bc; stats[FP_S_VALID] = rows.valid;
}

// arx_fastq_prepare.  What is refused is thrown: FsIoError, FsTooLarge, FsBadArg
inline void fp_files(int device, const char *const in_path[2], const char *const out_path[2], int format, int flags, int64_t max_bytes, int64_t run_bytes, const char *tmp_dir,
                     int64_t *stats, std::shared_ptr<DeviceBgzf> (*get_z)(int))
{
	const bool check = (flags & ARX_FQSORT_CHECK) != 0, gunzip_device = (flags & ARX_FQSORT_GUNZIP_DEVICE) != 0;
	fs_probe_inputs(in_path);
	int fmt = format;
	int64_t decided = -1;
	FpRows rows;
	if (format == FQS_AUTO) {
		{
			select_device(device, FP_NO_DEVICE);
			Stream st;
			st.create();
			FpHipDrv drv; drv.st = st;
			FqsCounts d;
			fqs_detect_files(drv, in_path, d, gunzip_device);
			fmt = d.format; decided = d.decided;
		}
		if (fmt == FQS_UNKNOWN) {
			fp_stats(stats, fmt, -1, rows);
			throw FsBadArg(fqs_no_format());
		}
		if (fmt == FQS_STANDARD) { // nothing to standardize: the sort itself, which leaves stats[24 ..] alone
			fp_stats(stats, fmt, decided, rows);
			if (run_bytes == 0) fs_sort_files(device, in_path, out_path, flags, max_bytes, stats, get_z);
			else fx_sort_files(device, in_path, out_path, flags, max_bytes, run_bytes, tmp_dir, stats, get_z);
			return;
		}
	}
	rows.format = fmt;
	FsFileSink sink;
	sink.bgzf = (flags & ARX_FQSORT_BGZF) != 0;
	FxFileStore store;
	if (!check) {
		sink.open(out_path);
		if (run_bytes != 0) store.create(tmp_dir, out_path[0]);
	}
	select_device(device, FP_NO_DEVICE);
	Stream st; // the call's own; declared before the buffers, so that it has ended when they are freed
	st.create();
	FpHipDrv drv; drv.st = st; drv.timed = (flags & ARX_FQSORT_TIMED) != 0;
	FqsFiles files;
	files.open(in_path, drv, FS_READ_CHUNK, max_bytes, gunzip_device);
	FxFileSrc &src = files.src;
	if (!check) sink.begin(st, device, get_z);
	FsCounts c{};
	FsSortMem m{};
	FxRuns S;
	FxIo io;
	if (run_bytes == 0) {
		const FsText T = src.load();
		fs_run_by(drv, T, FS_WINDOW_DEFAULT, FS_SLAB_DEFAULT, check ? nullptr : &sink, c, m, rows);
	} else {
		const int64_t rb = run_bytes == -1 ? fx_auto_run_bytes(FS_WINDOW_DEFAULT, FP_AUTO_SHARE) : run_bytes;
		fx_run_by(drv, src, check ? nullptr : &store, check ? nullptr : &sink, rb, rb < FS_WINDOW_DEFAULT ? rb : FS_WINDOW_DEFAULT, FS_SLAB_DEFAULT, c, m, S, io, rows);
		for (int f = 0; f < 2; ++f) { files.in[f].gz.reset(); files.in[f].rd.reset(); }
	}
	if (!check) sink.end(drv);
	fx_stats(stats, drv, c, src.total[0], src.total[1], !check, S, io);
	fp_stats(stats, fmt, decided, rows);
}

} // namespace arx

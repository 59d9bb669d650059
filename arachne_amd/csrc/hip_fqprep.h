// hip_fqprep.h -- dev_fqprep.h on the GPU, and the driver behind arx_fastq_prepare and arx_selftest_fastq_prepare (arx_bgzf.hip): a haplotagging,
// stLFR or TELLseq FASTQ file pair standardized and sorted by barcode in one call -- the bytes of arx_fastq_sort_ex after arx_fastq_standardize,
// without the files between them.
//
// Everything it runs on is the sort's and the standardization's (hip_fqsort.h, hip_fqstd.h): k_fs_items<F> starts one item of a functor per
// thread through hip_launch under the functor's name (fp_fields and fp_gather beside fq_*, fs_*, fx_* and fqs_match), FxHipDrv supplies scans,
// reductions, the key sort and the buffers, FqsFiles / FxFileSrc bring the files in slab by slab (a BGZF file inflated on the device), FsFileSink
// takes the output slabs (plain text or device BGZF), FxFileStore and FxIo hold the sorted runs.  Detection is fqs_files' own: a pass over the
// head of the files through readers of their own, the files opened again for the work.
//
//   AUTO finds standard   the call is fs_sort_files / fx_sort_files on the inputs, stats[24 ..] added
//   run_bytes == 0        both raw texts into device memory (through the readers' slab texts, device to device), fs_parse, FpFieldsF, the
//                         order by the composed key, FpGatherF into the sink
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
};

inline void fp_stats(int64_t *stats, int format, int64_t decided, const FpRows &rows)
{
	if (!stats) return;
	stats[FP_S_FORMAT] = format; stats[FP_S_DECIDED] = decided; stats[FP_S_WITH_BC] = rows.with_bc; stats[FP_S_VALID] = rows.valid;
}

// table, fields, order and (sink != null) the composing gather of two raw texts in device memory: fs_run with the composed key
inline void fp_run(FpHipDrv &drv, const FsText &T, int64_t window, int64_t slab, FsSink *sink, FsCounts &c, FsSortMem &m, FpRows &rows)
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
	FpKey key{};
	const int64_t longest = fp_order(drv, T, N, rows, m, c, key);
	ARX_HIP_CHECK(hipStreamSynchronize(drv.st));
	if (!drv.timed) drv.us[FS_T_SORT] = bs_now_us() - t0;
	c.slabs = 0;
	if (!sink) return;
	t0 = bs_now_us();
	rows.gather(drv, T, key, N, m, slab, longest, *sink, c);
	sink->flush();
	if (!drv.timed) drv.us[FS_T_GATHER] = bs_now_us() - t0 - sink->us_consume;
}

// fqs_files' detection: 4 MiB of each file first, a whole window only where a record does not fit that.  -> ARX_OK and format / decided, or ARX_E_IO
inline int fp_detect_files(FpHipDrv &drv, const char *const in_path[2], int &format, int64_t &decided, std::string &err)
{
	FqsCounts d;
	for (const int64_t window : {FQS_DETECT_WINDOW, FS_WINDOW_DEFAULT}) {
		FqsFiles files;
		if (!files.open(in_path, drv, err, window == FQS_DETECT_WINDOW ? FQS_DETECT_CHUNK : FS_READ_CHUNK)) return ARX_E_IO;
		d = FqsCounts();
		const int rc = fqs_detect(drv, files.src, window, d);
		ARX_HIP_CHECK(hipStreamSynchronize(drv.st));
		if (rc == FS_E_TOO_LARGE && window != FS_WINDOW_DEFAULT) continue; // a record of the head does not fit the small window
		fqs_throw(rc, window);
		break;
	}
	format = d.format; decided = d.decided;
	return ARX_OK;
}

// -> ARX_*; err: the text.  get_z: the device's compressor (arx_bgzf.hip keeps one per device)
inline int fp_files(int device, const char *const in_path[2], const char *const out_path[2], int format, int flags, int64_t max_bytes, int64_t run_bytes, const char *tmp_dir,
                    int64_t *stats, std::string &err, std::shared_ptr<DeviceBgzf> (*get_z)(int))
{
	const bool check = (flags & ARX_FQSORT_CHECK) != 0;
	for (int f = 0; f < 2; ++f) { // a missing input is refused before the device is touched
		FILE *p = fopen(in_path[f], "rb");
		if (!p) { err = std::string("cannot read ") + in_path[f]; return ARX_E_IO; }
		fclose(p);
	}
	int fmt = format;
	int64_t decided = -1;
	FpRows rows;
	if (format == FQS_AUTO) {
		{
			select_device(device, FP_NO_DEVICE);
			Stream st;
			st.create();
			FpHipDrv drv; drv.st = st;
			if (const int rc = fp_detect_files(drv, in_path, fmt, decided, err)) return rc;
		}
		if (fmt == FQS_UNKNOWN) {
			fp_stats(stats, fmt, -1, rows);
			err = "no record of the first " + std::to_string(FQS_DETECT_RECORDS) + " names a format (standard, haplotagging, stLFR, TELLseq): pass the format";
			return ARX_E_ARG;
		}
		if (fmt == FQS_STANDARD) { // nothing to standardize: the sort itself
			const int rc = run_bytes == 0 ? fs_sort_files(device, in_path, out_path, flags, max_bytes, stats, err, get_z)
			                              : fx_sort_files(device, in_path, out_path, flags, max_bytes, run_bytes, tmp_dir, stats, err, get_z);
			fp_stats(stats, fmt, decided, rows);
			return rc;
		}
	}
	rows.format = fmt;
	FsFileSink sink;
	sink.bgzf = (flags & ARX_FQSORT_BGZF) != 0;
	FxFileStore store;
	if (!check) {
		for (int f = 0; f < 2; ++f)
			if (!sink.file[f].open(out_path[f])) { err = std::string("cannot write ") + sink.file[f].tmp; sink.file[f].tmp.clear(); return ARX_E_IO; }
		if (run_bytes != 0) {
			std::string dir = tmp_dir ? tmp_dir : out_path[0];
			if (!tmp_dir) { const size_t cut = dir.rfind('/'); dir = cut == std::string::npos ? "." : cut == 0 ? "/" : dir.substr(0, cut); }
			for (int f = 0; f < 2; ++f)
				if (!store.file[f].create(dir, f ? ".r2" : ".r1")) { err = "cannot write a temporary file under " + dir; return ARX_E_IO; }
		}
	}
	select_device(device, FP_NO_DEVICE);
	Stream st; // the call's own; declared before the buffers, so that it has ended when they are freed
	st.create();
	FpHipDrv drv; drv.st = st; drv.timed = (flags & ARX_FQSORT_TIMED) != 0;
	FqsFiles files;
	if (!files.open(in_path, drv, err)) return ARX_E_IO;
	FxFileSrc &src = files.src;
	src.max_bytes = max_bytes;
	if (!check) {
		sink.init(st);
		if (sink.bgzf) sink.z = get_z(device);
	}
	FsCounts c{};
	FsSortMem m{};
	FxRuns S;
	FxIo io;
	if (run_bytes == 0) {
		// the two raw texts into device memory, as much at a time as the readers hand over
		const int64_t step = (int64_t)(FS_READ_CHUNK * FS_READ_CHUNKS);
		for (int f = 0; f < 2; ++f) {
			FsInput &I = files.in[f];
			while (!src.ended(f)) {
				I.room(I.len + step, st);
				I.len += src.fill(f, I.text.as<uint8_t>() + I.len, step);
			}
		}
		ARX_HIP_CHECK(hipStreamSynchronize(st));
		for (int f = 0; f < 2; ++f) { files.in[f].rd.reset(); src.text[f].release(); }
		src.d_comp.release(); src.d_rows.release(); src.d_status.release();
		const FsText T = {files.in[0].text.as<uint8_t>(), files.in[1].text.as<uint8_t>(), files.in[0].len, files.in[1].len};
		fp_run(drv, T, FS_WINDOW_DEFAULT, FS_SLAB_DEFAULT, check ? nullptr : &sink, c, m, rows);
	} else {
		const int64_t rb = run_bytes == -1 ? fx_auto_run_bytes(FS_WINDOW_DEFAULT, FP_AUTO_SHARE) : run_bytes;
		fx_run_by(drv, src, check ? nullptr : &store, check ? nullptr : &sink, rb, rb < FS_WINDOW_DEFAULT ? rb : FS_WINDOW_DEFAULT, FS_SLAB_DEFAULT, c, m, S, io, rows);
		for (int f = 0; f < 2; ++f) files.in[f].rd.reset();
	}
	if (!check) {
		sink.finish();
		drv.us[FS_T_COMPRESS] = sink.us_compress; drv.us[FS_T_WRITE] = sink.us_write;
	}
	fx_stats(stats, drv, c, src.total[0], src.total[1], !check, S, io);
	fp_stats(stats, fmt, decided, rows);
	return ARX_OK;
}

} // namespace arx

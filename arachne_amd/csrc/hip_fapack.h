// hip_fapack.h -- dev_fapack.h on the GPU, and the driver behind arx_index_build_ex and arx_selftest_fasta_pack (arx_bgzf.hip): the reference
// FASTA read through the FASTQ calls' readers (hip_fqsort.h: FsInput -- a BGZF file as it is, inflated on the device by FsSlabUp / inflate_launch;
// plain text and ordinary gzip through zlib on the reader thread), packed window by window into the forward strand, the contig table and the
// hole table in device memory, .pac / .ann / .amb written by index_build.h's writers, and the strand handed to the device suffix sorter where it
// lies (arx_index.hip: product_bwt_sa_device).  Replaces the host loop of bns_fasta2bntseq (bntseq.c:227-328) that build_index restates.
//
// Everything it runs on is the sort's: k_fs_items<F> starts one item of a functor per thread through hip_launch under the functor's name
// (fa_maps, fa_count, fa_holes, fa_emit, fa_pack, ...), FsHipDrv supplies the sums and the work buffers; FaHipDrv adds the running maximum, the
// 64-bit sum and the buffers that live as long as the call.
//
// A window is a piece of at most FA_WINDOW_DEFAULT bytes of a reader's slab where the slab lies: nothing of the text is carried from window to
// window, so nothing is copied.  Device memory of a call: the whole .pac (grown by half when the inflated size was not known), one slab of text
// (32 MiB; of a BGZF file its compressed form as well), per window 2.5 bytes of scratch per text byte and one code byte per base, the contig and
// hole rows (40 and 24 bytes each).  The text of the headers is fetched piece by piece, one copy per header and window: a FASTA of very many
// short contigs pays for that.
#pragma once
#include <sys/stat.h>
#include "hip_fqsort.h"
#include "dev_fapack.h"
#include "index_build.h"

namespace arx {

// arx_index.hip
std::string product_bwt_sa_device(int device, const uint8_t *dpac, size_t pac_bytes, int64_t l_pac, const uint64_t cnt_fwd[4], const std::string &prefix, const char *suffix);

constexpr int FA_N_STATS = 14; // ARX_INDEX_N_STATS
constexpr const char *FA_NO_DEVICE = "no such HIP device: the FASTA pack of arx_index_build_ex runs on the GPU (there is no CPU fallback)";
struct FaRefused : std::runtime_error { using std::runtime_error::runtime_error; }; // what arx_index_build refuses too, with its texts

struct FaHipDrv : FsHipDrv {
	DevBuf keep_[FA_N_KEEP];
	void scanmax32(int32_t *a, int64_t n)
	{
		if (n <= 0) return;
		booked("fa_scanmax", [&]() { dev_two_pass(tmp, "rocprim::inclusive_scan", [&](void *t, size_t &tb) { return rocprim::inclusive_scan(t, tb, a, a, (size_t)n, rocprim::maximum<int32_t>(), st); }); });
	}
	uint64_t sum64(const uint64_t *in, int64_t n) { return reduce("fa_sum", in, n, rocprim::plus<uint64_t>()); }
	// grows by half, as the sort's table; 64 bytes of room always stand behind `bytes` (the suffix sorter reads its text in words)
	void *keep(int which, int64_t bytes, int64_t kept)
	{
		DevBuf &b = keep_[which];
		if (!b.p || (size_t)bytes + 64 > b.bytes) {
			DevBuf t((size_t)(bytes + bytes / 2) + 64);
			if (b.p && kept > 0) ARX_HIP_CHECK(hipMemcpyAsync(t.p, b.p, (size_t)kept, hipMemcpyDeviceToDevice, st));
			ARX_HIP_CHECK(hipStreamSynchronize(st));
			b = std::move(t);
		}
		return b.p;
	}
	void reserve(int which, int64_t bytes) { if (!keep_[which].p) keep_[which].alloc((size_t)bytes + 64); }
	void release_work() // what only the pack needed makes room for the suffix sort
	{
		ARX_HIP_CHECK(hipStreamSynchronize(st));
		for (DevBuf &b : work_) b.release();
		for (int k = 0; k < FA_N_KEEP; ++k) if (k != FA_K_PAC) keep_[k].release();
		tmp.buf.release();
	}
};

// what a finished pack refuses
inline void fa_judge(const FaState &S)
{
	if (S.bad_start) throw FaRefused("FASTA does not start with '>'");
	if (S.l_pac == 0) throw FaRefused("empty FASTA");
	if (S.contig_too_long) throw FsTooLarge("a contig has more than 2147483647 bases: the index format has 32 bits for a contig's length");
}
inline void fa_count_check(int rc)
{
	if (rc == FA_E_COUNT) throw FsTooLarge("more than 2147483647 contigs or holes: the index format has 32 bits for their counts");
}

// the files of a call: each is written as <name>.tmp; commit() renames them all, and what was not committed is removed
struct FaOutFiles {
	std::vector<std::string> names;
	bool done = false;
	std::string add(const std::string &name) { names.push_back(name); return name + ".tmp"; }
	void commit()
	{
		for (const std::string &n : names)
			if (rename((n + ".tmp").c_str(), n.c_str()) != 0) throw FsIoError("cannot write " + n);
		done = true;
	}
	~FaOutFiles()
	{
		if (done) return;
		for (const std::string &n : names) (void)remove((n + ".tmp").c_str());
	}
};

// arx_index_build_ex.  What is refused is thrown: FaRefused, FsIoError, FsTooLarge
inline void fa_build_files(int device, const char *fasta, const char *prefix_, int flags, int64_t *stats)
{
	const double t_start = bs_now_us();
	const std::string prefix = prefix_;
	double us_read = 0, us_up = 0, us_pack = 0, us_pac = 0, us_ann = 0, us_sa = 0;
	struct stat sb;
	if (stat(fasta, &sb) != 0) throw FsIoError(std::string("cannot read ") + fasta);
	FsInput in;
	in.bgzf = file_is_bgzf(fasta);
	if (in.bgzf) {
		if (!in.open_as<BgzfChunkReader>(fasta, FS_READ_CHUNK)) throw FsIoError(std::string("cannot read ") + fasta);
	} else { // zlib; a gzip stream that ends inside a member is a read error here, not a shorter genome
		std::unique_ptr<ChunkReader> r(new ChunkReader());
		r->strict_end = true;
		const bool ok = r->open(fasta, FS_READ_CHUNK, FS_READ_CHUNKS);
		in.rd = std::move(r);
		if (!ok) throw FsIoError(std::string("cannot read ") + fasta);
	}
	FaOutFiles out;
	FILE *fpac = fopen(out.add(prefix + ".pac").c_str(), "wb");
	if (!fpac) { out.names.clear(); throw FsIoError("cannot write " + prefix + ".pac"); } // nothing was created
	struct Closer { FILE *&f; ~Closer() { if (f) fclose(f); } } closer{fpac};
	select_device(device, FA_NO_DEVICE);
	Stream st; // the call's own; declared before the buffers, so that it has ended when they are freed
	st.create();
	FaHipDrv drv; drv.st = st;
	const bool compressed = in.bgzf || file_is_gzip(fasta);
	drv.reserve(FA_K_PAC, compressed ? (int64_t)sb.st_size : (int64_t)sb.st_size / 4 + 1); // a genome deflates to about a quarter
	FaState S;
	FsSlabUp up;
	in.rd->start();
	int64_t text_bytes = 0;
	for (;;) {
		double t0 = bs_now_us();
		const SlabReader::Slab *s = in.rd->acquire();
		us_read += bs_now_us() - t0;
		if (!s) break;
		t0 = bs_now_us();
		if (s->err) throw FsIoError(std::string(fasta) + (in.bgzf ? ": not a chain of whole BGZF blocks" : ": read error (zlib reports a damaged or truncated stream)"));
		const int64_t n = (int64_t)s->text;
		uint8_t *text = (uint8_t *)drv.work(FA_W_TEXT, (n + 15) / 16 * 16 + 64);
		up.run(st, *s, in.bgzf, text, fasta);
		in.rd->release();
		text_bytes += n;
		us_up += bs_now_us() - t0;
		t0 = bs_now_us();
		for (int64_t a = 0; a < n; a += FA_WINDOW_DEFAULT) {
			fa_count_check(fa_window(drv, S, text + a, n - a < FA_WINDOW_DEFAULT ? n - a : FA_WINDOW_DEFAULT));
			if (S.bad_start) fa_judge(S);
		}
		us_pack += bs_now_us() - t0;
	}
	in.rd.reset();
	up.release();
	double t0 = bs_now_us();
	std::vector<FaContig> contigs;
	std::vector<FaHole> holes;
	fa_finish(drv, S, contigs, holes);
	fa_judge(S);
	us_pack += bs_now_us() - t0;
	// .pac: the packed bases through page-locked memory, then its end
	t0 = bs_now_us();
	const uint8_t *dpac = (const uint8_t *)drv.keep(FA_K_PAC, S.pac_bytes(), S.pac_bytes());
	{
		const size_t CH = (size_t)32 << 20, total = (size_t)S.pac_bytes();
		PinnedBuf pin(CH < total ? CH : total);
		for (size_t at = 0; at < total; at += CH) {
			const size_t k = total - at < CH ? total - at : CH;
			drv.fetch(pin.p, dpac + at, k);
			if (fwrite(pin.p, 1, k, fpac) != k) throw FsIoError("cannot write " + prefix + ".pac");
		}
		fa_write_pac_end(fpac, S.l_pac);
		FILE *f = fpac;
		fpac = nullptr;
		if (fclose(f) != 0) throw FsIoError("cannot write " + prefix + ".pac");
	}
	us_pac = bs_now_us() - t0;
	// .ann and .amb: the header texts and the rows through the host builder's own text handling and writers
	t0 = bs_now_us();
	{
		if ((int64_t)S.headers.size() != S.n_contigs) throw std::runtime_error("index build: the header texts and the contig rows disagree (internal error)");
		std::vector<FaAnn> anns;
		std::vector<FaAmb> ambs;
		anns.reserve(contigs.size()); ambs.reserve(holes.size());
		for (size_t c = 0; c < contigs.size(); ++c) {
			FaAnn a = fa_ann_of_header(S.headers[c], contigs[c].off);
			a.len = contigs[c].len; a.n_ambs = contigs[c].n_holes;
			anns.push_back(a);
		}
		for (const FaHole &h : holes) ambs.push_back(FaAmb{h.off, h.len, (char)h.ch});
		out.add(prefix + ".ann"); out.add(prefix + ".amb");
		const std::string e = fa_write_ann_amb(prefix, ".tmp", S.l_pac, anns, ambs);
		if (!e.empty()) throw FsIoError(e);
	}
	us_ann = bs_now_us() - t0;
	if (!(flags & ARX_INDEX_PACK_ONLY)) {
		t0 = bs_now_us();
		drv.release_work();
		out.add(prefix + ".bwt"); out.add(prefix + ".sa");
		const std::string e = product_bwt_sa_device(device, dpac, (size_t)S.pac_bytes(), S.l_pac, S.cnt, prefix, ".tmp");
		if (!e.empty()) throw std::runtime_error(e);
		ARX_HIP_CHECK(hipSetDevice(device));
		us_sa = bs_now_us() - t0;
	}
	out.commit();
	if (stats) {
		const int64_t v[FA_N_STATS] = {S.l_pac, S.n_contigs, S.n_holes, S.n_amb, text_bytes, (int64_t)sb.st_size, S.windows, (int64_t)us_read, (int64_t)us_up, (int64_t)us_pack,
		                               (int64_t)us_pac, (int64_t)us_ann, (int64_t)us_sa, (int64_t)(bs_now_us() - t_start)};
		for (int k = 0; k < FA_N_STATS; ++k) stats[k] = v[k];
	}
}

// arx_selftest_fasta_pack's pack: text[0, n) in host memory, in windows of `window` bytes
inline void fa_pack_mem(FaHipDrv &drv, const uint8_t *text, int64_t n, int64_t window, FaState &S, std::vector<FaContig> &contigs, std::vector<FaHole> &holes, std::vector<uint8_t> &pac)
{
	for (int64_t a = 0; a < n; a += window) {
		const int64_t k = n - a < window ? n - a : window;
		uint8_t *t = (uint8_t *)drv.work(FA_W_TEXT, (k + 15) / 16 * 16);
		ARX_HIP_CHECK(hipMemcpyAsync(t, text + a, (size_t)k, hipMemcpyHostToDevice, drv.st));
		ARX_HIP_CHECK(hipStreamSynchronize(drv.st));
		fa_count_check(fa_window(drv, S, t, k));
	}
	fa_finish(drv, S, contigs, holes);
	pac.assign((size_t)S.pac_bytes(), 0);
	if (!pac.empty()) drv.fetch(pac.data(), drv.keep(FA_K_PAC, S.pac_bytes(), S.pac_bytes()), pac.size());
}

} // namespace arx

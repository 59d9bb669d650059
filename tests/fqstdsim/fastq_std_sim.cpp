// tests/fqstdsim/fastq_std_sim.cpp -- TEST PROGRAM, not part of the product: arachne_amd/csrc/dev_fqstd.h (and through it the feeder's functors of
// dev_fastq.h, FsWindowF of dev_fqsort.h and bs_copy of dev_bamsort.h) compiled for the host, the items of a launch run one after the other in a
// loop.  tests/test_fastq_standardize_sim.py builds it with -fsanitize=address,undefined and runs it as a plain process.
//
//   fastq_std_sim MANIFEST OUTDIR     MANIFEST: one case per line, "name r1_path r2_path format claim,claim,..." (format: ARX_FQSTD_* 0 .. 3;
//                                     "-": no claim).  Every case runs at window_bytes FS_MIN_WINDOW, 256 and 4096, at slab_bytes 1 (one record
//                                     a slab) and 4096, the items of every launch in ascending and in descending order: twelve runs, every
//                                     buffer an allocation of exactly the bytes the orchestration asks its driver for, which must agree in
//                                     everything they report.  OUTDIR/name.r1 and .r2: the rewritten texts
// Prints per case "case name status format decided written records skipped with_barcode valid longest_barcode", and where something was written
// "off1 ..." and "off2 ..." (the records + 1 offsets of the records in the two outputs).  status 1: a line or a record does not fit the smallest
// window (then only that is reported).  format: the one used or found; written 0: the detection found standard or unknown.
// Exit status 3: two runs disagree; 4: a case did not meet a condition its line claims:
//   windows   more than one window was parsed at the smallest window size          skipped   lines were skipped
//   slabs     more than one slab at 4096 bytes
//   wide      (no condition) a record of the case fits no window below 1024 bytes: it runs at 1024, 2048 and 4096 instead
//   align     at 4096-byte slabs the records started at all 16 alignments in each output and their lines 2-4 at all 16 in each window
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sstream>
#include <string>
#include <vector>
#include "../../arachne_amd/csrc/dev_fqstd.h"

using namespace arx;

static void *exact(int64_t bytes) // an allocation of exactly `bytes`, 16-byte aligned: an access past it is the sanitizer's to find
{
	void *p = nullptr;
	if (posix_memalign(&p, 16, (size_t)bytes)) { fprintf(stderr, "out of memory\n"); exit(2); }
	if (bytes) memset(p, 0xA5, (size_t)bytes);
	return p;
}

struct SimDrv {
	bool rev = false;
	void *work_[FS_N_WORK] = {nullptr};
	~SimDrv() { for (void *p : work_) free(p); }
	template <class F> void items(const char *, int64_t n, const F &f)
	{
		if (rev) for (int64_t i = n - 1; i >= 0; --i) f(i);
		else for (int64_t i = 0; i < n; ++i) f(i);
	}
	void scan(const int64_t *in, int64_t *out, int64_t n) { int64_t a = 0; for (int64_t i = 0; i < n; ++i) { out[i] = a; a += in[i]; } out[n] = a; }
	int64_t scan32(const int32_t *in, int32_t *out, int64_t n) { int64_t a = 0; for (int64_t i = 0; i < n; ++i) { out[i] = (int32_t)a; a += in[i]; } out[n] = (int32_t)a; return a; }
	uint64_t max64(const uint64_t *in, int64_t n) { uint64_t m = 0; for (int64_t i = 0; i < n; ++i) m = in[i] > m ? in[i] : m; return m; }
	int64_t get(const int64_t *p) { return *p; }
	int32_t get32(const int32_t *p) { return *p; }
	void fetch(void *host, const void *dev, size_t bytes) { memcpy(host, dev, bytes); }
	void *work(int slot, int64_t bytes) { free(work_[slot]); work_[slot] = exact(bytes); return work_[slot]; }
	void phase(int) {}
};

struct SimSrc { // two texts in memory
	const std::vector<uint8_t> *t[2];
	int64_t at[2] = {0, 0};
	bool ended(int f) const { return at[f] == (int64_t)t[f]->size(); }
	int64_t fill(int f, uint8_t *dst, int64_t want)
	{
		const int64_t left = (int64_t)t[f]->size() - at[f], k = want < left ? want : left;
		if (k > 0) memcpy(dst, t[f]->data() + at[f], (size_t)k);
		at[f] += k;
		return k;
	}
};

struct SimSink { // every slab into two allocations of exactly its bytes; the alignments the composes met
	std::vector<uint8_t> out1, out2;
	uint8_t *d1 = nullptr, *d2 = nullptr;
	const SimDrv *drv = nullptr;
	bool dst_seen[2][16] = {}, src_seen[2][16] = {};
	void take(int64_t, int64_t cap, int64_t b1, int64_t b2, uint8_t **p1, uint8_t **p2)
	{
		if (b1 > cap || b2 > cap) { fprintf(stderr, "a slab of %lld / %lld bytes, more than the %lld promised\n", (long long)b1, (long long)b2, (long long)cap); exit(3); }
		*p1 = d1 = (uint8_t *)exact(b1); *p2 = d2 = (uint8_t *)exact(b2);
	}
	void give(int64_t, int64_t j0, int64_t j1, int64_t b1, int64_t b2)
	{
		const FqsRec *fld = (const FqsRec *)drv->work_[FQS_W_FLD];
		const int64_t *o1 = (const int64_t *)drv->work_[FQS_W_O1], *o2 = (const int64_t *)drv->work_[FQS_W_O2];
		for (int64_t j = j0; j < j1; ++j) {
			dst_seen[0][(o1[j] - o1[j0]) & 15] = true; dst_seen[1][(o2[j] - o2[j0]) & 15] = true;
			src_seen[0][fld[j].body1 & 15] = true; src_seen[1][fld[j].body2 & 15] = true;
		}
		out1.insert(out1.end(), d1, d1 + b1); out2.insert(out2.end(), d2, d2 + b2);
		free(d1); free(d2); d1 = d2 = nullptr;
	}
	bool all_alignments() const
	{
		for (int f = 0; f < 2; ++f)
			for (int a = 0; a < 16; ++a)
				if (!dst_seen[f][a] || !src_seen[f][a]) return false;
		return true;
	}
};

struct Result {
	int status = 0, format = 0, written = 0;
	int64_t decided = -1, windows = 0;
	FqsCounts c;
	std::vector<uint8_t> out1, out2;
	std::vector<int64_t> off1, off2;
	bool aligned = false;
};

static std::vector<uint8_t> slurp(const std::string &path)
{
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
	std::vector<uint8_t> v;
	uint8_t buf[65536];
	for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
	fclose(f);
	return v;
}

// what arx_fastq_standardize does with a format argument: detection where it is ARX_FQSTD_AUTO, then the conversion unless that found standard or unknown
static Result run(const std::vector<uint8_t> &in1, const std::vector<uint8_t> &in2, int format, int64_t window, int64_t slab, bool rev)
{
	Result r;
	r.format = format;
	if (format == FQS_AUTO) {
		SimDrv drv; drv.rev = rev;
		SimSrc src; src.t[0] = &in1; src.t[1] = &in2;
		FqsCounts d;
		r.status = fqs_detect(drv, src, window, d);
		if (r.status != FS_OK) return r;
		r.format = d.format; r.decided = d.decided;
		if (d.format == FQS_STANDARD || d.format == FQS_UNKNOWN) return r;
	}
	SimDrv drv; drv.rev = rev;
	SimSrc src; src.t[0] = &in1; src.t[1] = &in2;
	SimSink sink; sink.drv = &drv;
	r.c.off1 = &r.off1; r.c.off2 = &r.off2;
	r.status = fqs_convert(drv, src, r.format, window, slab, sink, r.c);
	r.c.off1 = r.c.off2 = nullptr;
	if (r.status != FS_OK) return r;
	r.written = 1;
	r.out1.swap(sink.out1); r.out2.swap(sink.out2);
	r.aligned = sink.all_alignments();
	return r;
}

int main(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: fastq_std_sim MANIFEST OUTDIR\n"); return 2; }
	FILE *mf = fopen(argv[1], "r");
	if (!mf) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
	char line[4096];
	while (fgets(line, sizeof line, mf)) {
		std::istringstream ls(line);
		std::string name, p1, p2, claims;
		int format = 0;
		if (!(ls >> name >> p1 >> p2 >> format >> claims)) continue;
		if (format < FQS_AUTO || format > FQS_TELLSEQ) { fprintf(stderr, "%s: format %d\n", name.c_str(), format); return 2; }
		const std::vector<uint8_t> in1 = slurp(p1), in2 = slurp(p2);
		Result first;
		bool have = false, many_windows = false, many_slabs = false, aligned = false;
		const bool wide = ("," + claims + ",").find(",wide,") != std::string::npos;
		const int64_t smallest = wide ? 1024 : FS_MIN_WINDOW;
		for (int64_t window : {smallest, 2 * smallest, (int64_t)4096})
			for (int64_t slab : {(int64_t)1, (int64_t)4096})
				for (int rev = 0; rev < 2; ++rev) {
					Result r = run(in1, in2, format, window, slab, rev != 0);
					if (window == smallest && r.c.windows > 1) many_windows = true;
					if (slab == 4096 && r.c.slabs > 1) many_slabs = true;
					if (slab == 4096 && r.aligned) aligned = true;
					if (slab == 1 && r.written && r.c.slabs != r.c.n_records) { fprintf(stderr, "%s: %lld slabs of one record for %lld records\n", name.c_str(), (long long)r.c.slabs, (long long)r.c.n_records); return 3; }
					if (!have) { first = std::move(r); have = true; continue; }
					const FqsCounts &a = r.c, &b = first.c;
					if (r.status != FS_OK && r.status == first.status) continue; // refused alike: how far each got is its window's business
					if (r.status != first.status || r.format != first.format || r.decided != first.decided || r.written != first.written || a.n_records != b.n_records || a.skipped != b.skipped ||
					    a.with_bc != b.with_bc || a.valid != b.valid || a.max_bc != b.max_bc || a.bytes1 != b.bytes1 || a.bytes2 != b.bytes2 ||
					    r.out1 != first.out1 || r.out2 != first.out2 || r.off1 != first.off1 || r.off2 != first.off2) {
						fprintf(stderr, "%s: window %lld slab %lld rev %d disagrees with the first run (status %d / %d, format %d / %d, records %lld / %lld)\n", name.c_str(), (long long)window,
						        (long long)slab, rev, r.status, first.status, r.format, first.format, (long long)a.n_records, (long long)b.n_records);
						return 3;
					}
				}
		std::istringstream cs(claims);
		for (std::string c; std::getline(cs, c, ',');) {
			bool ok = true;
			if (c == "windows") ok = many_windows;
			else if (c == "slabs") ok = many_slabs;
			else if (c == "skipped") ok = first.c.skipped > 0;
			else if (c == "align") ok = aligned;
			else if (c == "wide") ok = true;
			else if (c != "-") { fprintf(stderr, "%s: unknown claim %s\n", name.c_str(), c.c_str()); return 2; }
			if (!ok) { fprintf(stderr, "%s does not meet its claim: %s\n", name.c_str(), c.c_str()); return 4; }
		}
		const FqsCounts &c = first.c;
		printf("case %s %d %d %lld %d %lld %lld %lld %lld %lld\n", name.c_str(), first.status, first.format, (long long)first.decided, first.written, (long long)c.n_records, (long long)c.skipped,
		       (long long)c.with_bc, (long long)c.valid, (long long)c.max_bc);
		if (first.status != FS_OK || !first.written) continue;
		for (int f = 0; f < 2; ++f) {
			printf(f ? "off2" : "off1");
			for (int64_t x : f ? first.off2 : first.off1) printf(" %lld", (long long)x);
			printf("\n");
			const std::string path = std::string(argv[2]) + "/" + name + (f ? ".r2" : ".r1");
			FILE *o = fopen(path.c_str(), "wb");
			if (!o) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 2; }
			const std::vector<uint8_t> &out = f ? first.out2 : first.out1;
			if (!out.empty()) fwrite(out.data(), 1, out.size(), o);
			fclose(o);
		}
	}
	fclose(mf);
	return 0;
}

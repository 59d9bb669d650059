// tests/fqprepsim/fastq_prepare_sim.cpp -- TEST PROGRAM, not part of the product: arachne_amd/csrc/dev_fqprep.h (the header standardization fused
// into the FASTQ sort) and through it dev_fqstd.h, dev_fqsort.h and dev_fqmerge.h compiled for the host, the items of a launch run one after the
// other in a loop, the key sort by std::stable_sort, the run files two vectors.  tests/test_fastq_prepare_sim.py builds it with
// -fsanitize=address,undefined and runs it as a plain process.
//
//   fastq_prepare_sim MANIFEST OUTDIR   MANIFEST: one line per case and run size, "name r1_path r2_path format run_bytes w1,w2,w3".  Every line is
//                                       run at its three windows (a run's window is at most run_bytes), slab_bytes 1 and 4096, the items of
//                                       every launch ascending and descending -- twelve runs that must agree in everything they report but the
//                                       windows.  run_bytes 0: both texts in memory whole.  Every buffer -- texts, run buffers, stage buffers, the
//                                       tables and the key buffer among them -- is an allocation of exactly the bytes the orchestration asks for.
//                                       OUTDIR/name.run_bytes.r1 and .r2: the prepared texts
// Prints per line "case name run_bytes status format decided records skipped runs distinct longest_key with_barcode valid sorted_runs", and for
// status 0 "off1 ..." and "off2 ...".  status: the FS_E_* of dev_fqsort.h and dev_fqmerge.h; 9: detection found no format.
// Exit status 3: two runs disagree, or the merge did not read every byte of the run files exactly once, front to back per run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>
#include "../../arachne_amd/csrc/dev_fqprep.h"

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
	void *work_[FS_N_WORK] = {nullptr}, *run_[2] = {nullptr, nullptr}, *keep_[2] = {nullptr, nullptr};
	FsRec *tab_ = nullptr; int64_t tab_n_ = 0;
	~SimDrv() { for (void *p : work_) free(p); for (void *p : run_) free(p); for (void *p : keep_) free(p); free(tab_); }
	template <class F> void items(const char *, int64_t n, const F &f)
	{
		if (rev) for (int64_t i = n - 1; i >= 0; --i) f(i);
		else for (int64_t i = 0; i < n; ++i) f(i);
	}
	void phase(int) {}
	void scan(const int64_t *in, int64_t *out, int64_t n) { int64_t a = 0; for (int64_t i = 0; i < n; ++i) { out[i] = a; a += in[i]; } out[n] = a; }
	int64_t scan32(const int32_t *in, int32_t *out, int64_t n) { int64_t a = 0; for (int64_t i = 0; i < n; ++i) { out[i] = (int32_t)a; a += in[i]; } out[n] = (int32_t)a; return a; }
	uint64_t max64(const uint64_t *in, int64_t n) { uint64_t m = 0; for (int64_t i = 0; i < n; ++i) m = in[i] > m ? in[i] : m; return m; }
	uint64_t or64(const uint64_t *in, int64_t n) { uint64_t m = 0; for (int64_t i = 0; i < n; ++i) m |= in[i]; return m; }
	int64_t get(const int64_t *p) { return *p; }
	int32_t get32(const int32_t *p) { return *p; }
	void fetch(void *host, const void *dev, size_t bytes) { memcpy(host, dev, bytes); }
	void upload(void *dev, const void *host, size_t bytes) { memcpy(dev, host, bytes); }
	void copy(void *dst, const void *src, int64_t n)
	{
		const uint8_t *s = (const uint8_t *)src, *d = (const uint8_t *)dst;
		if (s < d + n && d < s + n) { fprintf(stderr, "an overlapping copy of %lld bytes\n", (long long)n); exit(3); }
		memcpy(dst, src, (size_t)n);
	}
	void sort_pairs(const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, int64_t n, int bits)
	{
		const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1;
		std::vector<int64_t> idx((size_t)n);
		std::iota(idx.begin(), idx.end(), (int64_t)0);
		std::stable_sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return (kin[a] & mask) < (kin[b] & mask); });
		for (int64_t i = 0; i < n; ++i) { kout[i] = kin[idx[(size_t)i]]; vout[i] = vin[idx[(size_t)i]]; }
	}
	void *work(int slot, int64_t bytes) { free(work_[slot]); work_[slot] = exact(bytes); return work_[slot]; }
	void *run_buf(int f, int64_t bytes) { free(run_[f]); run_[f] = exact(bytes); return run_[f]; }
	void *keep(int which, int64_t bytes, int64_t kept)
	{
		void *p = exact(bytes);
		if (kept) memcpy(p, keep_[which], (size_t)kept);
		free(keep_[which]);
		return keep_[which] = p;
	}
	FsRec *table(int64_t n)
	{
		if (n <= tab_n_) return tab_;
		const int64_t room = fs_table_room(n);
		FsRec *t = (FsRec *)exact(room * (int64_t)sizeof(FsRec));
		if (tab_n_) memcpy(t, tab_, (size_t)tab_n_ * sizeof(FsRec));
		free(tab_);
		tab_ = t; tab_n_ = room;
		return t;
	}
};

struct SimSrc {
	const std::vector<uint8_t> *in[2];
	size_t at[2] = {0, 0};
	bool ended(int f) const { return at[f] == in[f]->size(); }
	int64_t fill(int f, uint8_t *dst, int64_t want)
	{
		const size_t n = std::min((size_t)want, in[f]->size() - at[f]);
		if (n) memcpy(dst, in[f]->data() + at[f], n);
		at[f] += n;
		return (int64_t)n;
	}
};

struct SimSlabs { // every slab into two allocations of exactly its bytes
	std::vector<uint8_t> text[2];
	uint8_t *d[2] = {nullptr, nullptr};
	void take(int64_t, int64_t cap, int64_t b1, int64_t b2, uint8_t **p1, uint8_t **p2)
	{
		if (b1 > cap || b2 > cap) { fprintf(stderr, "a slab of %lld / %lld bytes, more than the %lld promised\n", (long long)b1, (long long)b2, (long long)cap); exit(3); }
		*p1 = d[0] = (uint8_t *)exact(b1); *p2 = d[1] = (uint8_t *)exact(b2);
	}
	void give(int64_t, int64_t, int64_t, int64_t b1, int64_t b2)
	{
		text[0].insert(text[0].end(), d[0], d[0] + b1); text[1].insert(text[1].end(), d[1], d[1] + b2);
		free(d[0]); free(d[1]); d[0] = d[1] = nullptr;
	}
};
struct SimIo : SimSlabs { // the run files: text[f]; what the merge read of them
	std::vector<int64_t> run_end[2]; // where the runs end in the files
	std::vector<int64_t> next[2];    // per run: the next byte the merge may read
	int64_t n_read[2] = {0, 0};
	void end_run() { for (int f = 0; f < 2; ++f) { next[f].push_back(run_end[f].empty() ? 0 : run_end[f].back()); run_end[f].push_back((int64_t)text[f].size()); } }
	void begin(int64_t) {}
	void read(int f, int64_t at, int64_t n, uint8_t *dst)
	{
		const size_t r = (size_t)(std::upper_bound(run_end[f].begin(), run_end[f].end(), at) - run_end[f].begin());
		if (r >= next[f].size() || at != next[f][r] || at + n > run_end[f][r]) { fprintf(stderr, "run file %d: bytes [%lld, %lld) are not the next of their run\n", f, (long long)at, (long long)(at + n)); exit(3); }
		next[f][r] = at + n; n_read[f] += n;
		memcpy(dst, text[f].data() + at, (size_t)n);
	}
	void staged() {}
};

enum { SIM_UNKNOWN = 9 };
struct Result {
	int status = 0, format = 0;
	int64_t decided = -1, with_bc = 0, valid = 0, n_runs = 0;
	FsCounts c{};
	std::vector<uint8_t> out1, out2;
	std::vector<int64_t> off1, off2;
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

static Result run(const std::vector<uint8_t> &in1, const std::vector<uint8_t> &in2, int format, int64_t run_bytes, int64_t window, int64_t slab, bool rev)
{
	Result r;
	SimDrv drv; drv.rev = rev;
	r.format = format;
	if (format == FQS_AUTO) { // a pass of its own
		SimSrc src; src.in[0] = &in1; src.in[1] = &in2;
		FqsCounts d;
		r.status = fqs_detect(drv, src, window, d);
		if (r.status != FS_OK) return r;
		r.format = d.format; r.decided = d.decided;
		if (r.format == FQS_UNKNOWN) { r.status = SIM_UNKNOWN; return r; }
	}
	FpRows rows; rows.format = r.format;
	FxPlainRows plain;
	const bool standard = r.format == FQS_STANDARD;
	SimSlabs sink;
	FsSortMem m;
	if (run_bytes == 0) {
		uint8_t *t1 = (uint8_t *)exact((int64_t)in1.size()), *t2 = (uint8_t *)exact((int64_t)in2.size());
		if (!in1.empty()) memcpy(t1, in1.data(), in1.size());
		if (!in2.empty()) memcpy(t2, in2.data(), in2.size());
		const FsText T = {t1, t2, (int64_t)in1.size(), (int64_t)in2.size()};
		r.status = fs_parse(drv, T, window, r.c);
		if (r.status == FS_OK) {
			const int64_t N = r.c.n_records;
			if (standard) {
				fs_sort_mem(drv, N, m);
				const int64_t longest = fs_order(drv, T, drv.tab_, N, m, r.c);
				fs_gather(drv, T, drv.tab_, N, m, slab, longest, sink, r.c);
			} else {
				FpKey key{};
				const int64_t longest = fp_order(drv, T, N, rows, m, r.c, key);
				rows.gather(drv, T, key, N, m, slab, longest, sink, r.c);
			}
		}
		free(t1); free(t2);
		if (r.status != FS_OK) return r;
	} else {
		SimSrc src; src.in[0] = &in1; src.in[1] = &in2;
		SimIo io;
		FxRuns S;
		r.status = standard ? fx_runs_by(drv, src, &io, run_bytes, window, slab, S, plain) : fx_runs_by(drv, src, &io, run_bytes, window, slab, S, rows);
		if (r.status != FS_OK) return r;
		r.status = fx_merge(drv, &io, &sink, S, slab, m, r.c);
		if (r.status != FS_OK) return r;
		for (int f = 0; f < 2; ++f)
			if (io.n_read[f] != (int64_t)io.text[f].size()) { fprintf(stderr, "run file %d: %lld of %lld bytes were read\n", f, (long long)io.n_read[f], (long long)io.text[f].size()); exit(3); }
		r.n_runs = S.n_runs;
	}
	r.with_bc = rows.with_bc; r.valid = rows.valid;
	r.out1.swap(sink.text[0]); r.out2.swap(sink.text[1]);
	const int64_t N = r.c.n_records;
	if (N) { r.off1.assign(m.out1, m.out1 + N + 1); r.off2.assign(m.out2, m.out2 + N + 1); }
	else { r.off1.assign(1, 0); r.off2.assign(1, 0); }
	return r;
}

int main(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: fastq_prepare_sim MANIFEST OUTDIR\n"); return 2; }
	FILE *mf = fopen(argv[1], "r");
	if (!mf) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
	char line[4096];
	while (fgets(line, sizeof line, mf)) {
		std::istringstream ls(line);
		std::string name, p1, p2, ws;
		long long rb = 0, w[3] = {0, 0, 0};
		int format = 0;
		if (!(ls >> name >> p1 >> p2 >> format >> rb >> ws) || sscanf(ws.c_str(), "%lld,%lld,%lld", &w[0], &w[1], &w[2]) != 3) continue;
		const std::vector<uint8_t> in1 = slurp(p1), in2 = slurp(p2);
		Result first;
		bool have = false;
		for (long long win : w)
			for (int64_t slab : {(int64_t)1, (int64_t)4096})
				for (int rev = 0; rev < 2; ++rev) {
					const int64_t window = rb != 0 && rb < win ? rb : win;
					Result r = run(in1, in2, format, rb, window, slab, rev != 0);
					if (slab == 1 && r.status == FS_OK && r.c.slabs != r.c.n_records) { fprintf(stderr, "%s: %lld slabs of one record for %lld records\n", name.c_str(), (long long)r.c.slabs, (long long)r.c.n_records); return 3; }
					if (!have) { first = std::move(r); have = true; continue; }
					const FsCounts &a = r.c, &b = first.c;
					if (r.status != first.status || r.format != first.format || r.decided != first.decided || a.n_records != b.n_records || a.skipped != b.skipped ||
					    a.runs_in != b.runs_in || a.distinct != b.distinct || a.max_bc != b.max_bc || a.passes != b.passes || a.bytes1 != b.bytes1 || a.bytes2 != b.bytes2 ||
					    r.with_bc != first.with_bc || r.valid != first.valid || r.out1 != first.out1 || r.out2 != first.out2 || r.off1 != first.off1 || r.off2 != first.off2) {
						fprintf(stderr, "%s: run_bytes %lld window %lld slab %lld rev %d disagrees with the first run (status %d / %d, records %lld / %lld)\n", name.c_str(), rb, (long long)window,
						        (long long)slab, rev, r.status, first.status, (long long)a.n_records, (long long)b.n_records);
						return 3;
					}
				}
		const FsCounts &c = first.c;
		printf("case %s %lld %d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", name.c_str(), rb, first.status, first.format, (long long)first.decided, (long long)c.n_records,
		       (long long)c.skipped, (long long)c.runs_in, (long long)c.distinct, (long long)c.max_bc, (long long)first.with_bc, (long long)first.valid, (long long)first.n_runs);
		if (first.status != FS_OK) continue;
		for (int f = 0; f < 2; ++f) {
			printf(f ? "off2" : "off1");
			for (int64_t x : f ? first.off2 : first.off1) printf(" %lld", (long long)x);
			printf("\n");
			const std::string path = std::string(argv[2]) + "/" + name + "." + std::to_string(rb) + (f ? ".r2" : ".r1");
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

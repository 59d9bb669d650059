// tests/fqsortsim/fastq_sort_sim.cpp -- TEST PROGRAM, not part of the product: arachne_amd/csrc/dev_fqsort.h (and through it the feeder's functors of
// dev_fastq.h and bs_copy of dev_bamsort.h) compiled for the host, the items of a launch run one after the other in a loop, the key sort by
// std::stable_sort.  tests/test_fastq_sort_sim.py builds it with -fsanitize=address,undefined and runs it as a plain process.
//
//   fastq_sort_sim MANIFEST OUTDIR     MANIFEST: one case per line, "name r1_path r2_path claim,claim,..." ("-": no claim).  Every case runs at
//                                      window_bytes FS_MIN_WINDOW, 256 and 4096, at slab_bytes 1 (one record a slab) and 4096, the items of
//                                      every launch in ascending and in descending order: twelve runs, every buffer an allocation of exactly the
//                                      bytes the orchestration asks its driver for, which must agree in everything they report.
//                                      OUTDIR/name.r1 and .r2: the sorted texts
// Prints per case "case name status records skipped runs distinct longest_barcode", "off1 ..." and "off2 ..." (the records + 1 offsets of the
// sorted records in the two outputs).  status 1: a line or a record does not fit the smallest window (then only that is reported).
// Exit status 3: two runs disagree; 4: a case did not meet a condition its line claims:
//   windows   more than one window was parsed at the smallest window size          blocks    more than 256 records: two blocks of every per-record launch
//   slabs     more than one slab at 4096 bytes                                      chunks    a barcode of more than 16 bytes: three chunk passes at least
//   skipped   lines were skipped                                                    align     the gather copied at all 8 x 8 (source, destination)
//   large     more than 65536 records                                                         alignments mod 8 in each file
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>
#include "../../arachne_amd/csrc/dev_fqsort.h"

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
	FsRec *tab_ = nullptr; int64_t tab_n_ = 0;
	int64_t most_items = 0;
	~SimDrv() { for (void *p : work_) free(p); free(tab_); }
	template <class F> void items(const char *, int64_t n, const F &f)
	{
		if (n > most_items) most_items = n;
		if (rev) for (int64_t i = n - 1; i >= 0; --i) f(i);
		else for (int64_t i = 0; i < n; ++i) f(i);
	}
	void scan(const int64_t *in, int64_t *out, int64_t n) { int64_t a = 0; for (int64_t i = 0; i < n; ++i) { out[i] = a; a += in[i]; } out[n] = a; }
	int64_t scan32(const int32_t *in, int32_t *out, int64_t n) { int64_t a = 0; for (int64_t i = 0; i < n; ++i) { out[i] = (int32_t)a; a += in[i]; } out[n] = (int32_t)a; return a; }
	uint64_t max64(const uint64_t *in, int64_t n) { uint64_t m = 0; for (int64_t i = 0; i < n; ++i) m = in[i] > m ? in[i] : m; return m; }
	uint64_t or64(const uint64_t *in, int64_t n) { uint64_t m = 0; for (int64_t i = 0; i < n; ++i) m |= in[i]; return m; }
	int64_t get(const int64_t *p) { return *p; }
	int32_t get32(const int32_t *p) { return *p; }
	void fetch(void *host, const void *dev, size_t bytes) { memcpy(host, dev, bytes); }
	void sort_pairs(const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, int64_t n, int bits)
	{
		const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1;
		std::vector<int64_t> idx((size_t)n);
		std::iota(idx.begin(), idx.end(), (int64_t)0);
		std::stable_sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return (kin[a] & mask) < (kin[b] & mask); });
		for (int64_t i = 0; i < n; ++i) { kout[i] = kin[idx[(size_t)i]]; vout[i] = vin[idx[(size_t)i]]; }
	}
	void *work(int slot, int64_t bytes) { free(work_[slot]); work_[slot] = exact(bytes); return work_[slot]; }
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

struct SimSink { // every slab into two allocations of exactly its bytes; the alignments the copies met
	std::vector<uint8_t> out1, out2;
	uint8_t *d1 = nullptr, *d2 = nullptr;
	const FsText *T = nullptr; const FsRec *tab = nullptr; const FsSortMem *m = nullptr;
	bool seen[2][8][8] = {};
	void take(int64_t, int64_t cap, int64_t b1, int64_t b2, uint8_t **p1, uint8_t **p2)
	{
		if (b1 > cap || b2 > cap) { fprintf(stderr, "a slab of %lld / %lld bytes, more than the %lld promised\n", (long long)b1, (long long)b2, (long long)cap); exit(3); }
		*p1 = d1 = (uint8_t *)exact(b1); *p2 = d2 = (uint8_t *)exact(b2);
	}
	void give(int64_t, int64_t j0, int64_t j1, int64_t b1, int64_t b2)
	{
		for (int64_t j = j0; j < j1; ++j) {
			const FsRec &r = tab[m->vals[m->cur][j]];
			seen[0][(uintptr_t)(T->t1 + r.off1) & 7][(uintptr_t)(d1 + (m->out1[j] - m->out1[j0])) & 7] = true;
			seen[1][(uintptr_t)(T->t2 + r.off2) & 7][(uintptr_t)(d2 + (m->out2[j] - m->out2[j0])) & 7] = true;
		}
		out1.insert(out1.end(), d1, d1 + b1); out2.insert(out2.end(), d2, d2 + b2);
		free(d1); free(d2); d1 = d2 = nullptr;
	}
};

struct Result {
	int status = 0;
	FsCounts c{};
	std::vector<uint8_t> out1, out2;
	std::vector<int64_t> off1, off2;
	int64_t most_items = 0;
	bool seen[2][8][8] = {};
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

static Result run(const std::vector<uint8_t> &in1, const std::vector<uint8_t> &in2, int64_t window, int64_t slab, bool rev)
{
	Result r;
	uint8_t *t1 = (uint8_t *)exact((int64_t)in1.size()), *t2 = (uint8_t *)exact((int64_t)in2.size());
	if (!in1.empty()) memcpy(t1, in1.data(), in1.size());
	if (!in2.empty()) memcpy(t2, in2.data(), in2.size());
	{
		SimDrv drv; drv.rev = rev;
		const FsText T = {t1, t2, (int64_t)in1.size(), (int64_t)in2.size()};
		r.status = fs_parse(drv, T, window, r.c);
		if (r.status == FS_OK) {
			const int64_t N = r.c.n_records;
			FsSortMem m;
			fs_sort_mem(drv, N, m);
			const int64_t longest = fs_order(drv, T, drv.tab_, N, m, r.c);
			SimSink sink; sink.T = &T; sink.tab = drv.tab_; sink.m = &m;
			fs_gather(drv, T, drv.tab_, N, m, slab, longest, sink, r.c);
			r.out1.swap(sink.out1); r.out2.swap(sink.out2);
			if (N) { r.off1.assign(m.out1, m.out1 + N + 1); r.off2.assign(m.out2, m.out2 + N + 1); }
			else { r.off1.assign(1, 0); r.off2.assign(1, 0); }
			memcpy(r.seen, sink.seen, sizeof r.seen);
		}
		r.most_items = drv.most_items;
	}
	free(t1); free(t2);
	return r;
}

static bool all_alignments(const Result &r)
{
	for (int f = 0; f < 2; ++f)
		for (int a = 0; a < 8; ++a)
			for (int b = 0; b < 8; ++b)
				if (!r.seen[f][a][b]) return false;
	return true;
}

int main(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: fastq_sort_sim MANIFEST OUTDIR\n"); return 2; }
	FILE *mf = fopen(argv[1], "r");
	if (!mf) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
	char line[4096];
	while (fgets(line, sizeof line, mf)) {
		std::istringstream ls(line);
		std::string name, p1, p2, claims;
		if (!(ls >> name >> p1 >> p2 >> claims)) continue;
		const std::vector<uint8_t> in1 = slurp(p1), in2 = slurp(p2);
		Result first;
		bool have = false, many_windows = false, many_slabs = false, aligned = false;
		for (int64_t window : {FS_MIN_WINDOW, (int64_t)256, (int64_t)4096})
			for (int64_t slab : {(int64_t)1, (int64_t)4096})
				for (int rev = 0; rev < 2; ++rev) {
					Result r = run(in1, in2, window, slab, rev != 0);
					if (window == FS_MIN_WINDOW && r.c.windows > 1) many_windows = true;
					if (slab == 4096 && r.c.slabs > 1) many_slabs = true;
					if (slab == 1 && r.status == FS_OK && r.c.slabs != r.c.n_records) { fprintf(stderr, "%s: %lld slabs of one record for %lld records\n", name.c_str(), (long long)r.c.slabs, (long long)r.c.n_records); return 3; }
					if (all_alignments(r)) aligned = true;
					if (!have) { first = std::move(r); have = true; continue; }
					const FsCounts &a = r.c, &b = first.c;
					if (r.status != first.status || a.n_records != b.n_records || a.skipped != b.skipped || a.runs_in != b.runs_in || a.distinct != b.distinct || a.max_bc != b.max_bc ||
					    a.passes != b.passes || a.bytes1 != b.bytes1 || a.bytes2 != b.bytes2 || r.out1 != first.out1 || r.out2 != first.out2 || r.off1 != first.off1 || r.off2 != first.off2) {
						fprintf(stderr, "%s: window %lld slab %lld rev %d disagrees with the first run (status %d / %d, records %lld / %lld)\n", name.c_str(), (long long)window, (long long)slab, rev,
						        r.status, first.status, (long long)a.n_records, (long long)b.n_records);
						return 3;
					}
				}
		std::istringstream cs(claims);
		for (std::string c; std::getline(cs, c, ',');) {
			bool ok = true;
			if (c == "windows") ok = many_windows;
			else if (c == "blocks") ok = first.c.n_records > 256 && first.most_items > 256;
			else if (c == "slabs") ok = many_slabs;
			else if (c == "chunks") ok = first.c.max_bc > 16 && first.c.passes >= 3;
			else if (c == "skipped") ok = first.c.skipped > 0;
			else if (c == "align") ok = aligned;
			else if (c == "large") ok = first.c.n_records > 65536;
			else if (c != "-") { fprintf(stderr, "%s: unknown claim %s\n", name.c_str(), c.c_str()); return 2; }
			if (!ok) { fprintf(stderr, "%s does not meet its claim: %s\n", name.c_str(), c.c_str()); return 4; }
		}
		const FsCounts &c = first.c;
		printf("case %s %d %lld %lld %lld %lld %lld\n", name.c_str(), first.status, (long long)c.n_records, (long long)c.skipped, (long long)c.runs_in, (long long)c.distinct, (long long)c.max_bc);
		if (first.status != FS_OK) continue;
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

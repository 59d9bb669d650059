// tests/sortsim/bam_sort_sim.cpp -- TEST PROGRAM, not part of the product: arachne_amd/csrc/dev_bamsort.h compiled for the host, the items of a
// launch run one after the other in a loop, the key sort by std::stable_sort.  tests/test_bam_sort_sim.py builds it with
// -fsanitize=address,undefined and runs it as a plain process.
//
//   bam_sort_sim sort IN OUT N_REF      IN: plain BAM record bytes.  Discovery, keys, sort and gather at seg_bytes 64, 256 and 4096, the items
//                                       of every launch in ascending and in descending order: six runs, each from allocations of exactly the
//                                       sizes the product's driver uses, which must agree byte for byte.  OUT: the sorted bytes (0xA5
//                                       throughout where the chain is broken: nothing may have been written)
//   bam_sort_sim copy IN OUT N_REF SLAB the records counted slab by slab as the product's copy mode counts them, slabs of SLAB bytes cut
//                                       wherever that falls, each an allocation of exactly its bytes (and the three in front); the same six
//                                       runs.  OUT: nothing is written to it
//   bam_sort_sim time IN N_REF SEG      one sort at SEG, timed (tools/bam_sort_bench.py builds this program without the sanitizers for it)
// Prints "status S" (0, or 1: the chain is broken), "records N", one line "cfg seg rev segments right repaired rounds" per run and
// "rec_off ..." (sort: the N + 1 offsets of the sorted records).  Exit status 3: two runs disagree.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <numeric>
#include <vector>
#include "../../arachne_amd/csrc/dev_bamsort.h"

using namespace arx;

struct SimDrv {
	bool rev = false;
	template <class F> void items(const char *, int64_t n, const F &f)
	{
		if (rev) for (int64_t i = n - 1; i >= 0; --i) f(i);
		else for (int64_t i = 0; i < n; ++i) f(i);
	}
	void scan(const int64_t *in, int64_t *out, int64_t n) { int64_t a = 0; for (int64_t i = 0; i < n; ++i) { out[i] = a; a += in[i]; } out[n] = a; }
	int64_t get(const int64_t *p) { return *p; }
	void put(int64_t *p, int64_t v) { *p = v; }
	void sort_pairs(const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, int64_t n, int bits)
	{
		const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1;
		std::vector<int64_t> idx((size_t)n);
		std::iota(idx.begin(), idx.end(), (int64_t)0);
		std::stable_sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return (kin[a] & mask) < (kin[b] & mask); });
		for (int64_t i = 0; i < n; ++i) { kout[i] = kin[idx[(size_t)i]]; vout[i] = vin[idx[(size_t)i]]; }
	}
};

struct Result { int status = 0; int64_t n_records = 0; std::vector<uint8_t> out; std::vector<int64_t> rec_off; BsFound f{}; };

static std::vector<uint8_t> slurp(const char *path)
{
	FILE *f = fopen(path, "rb");
	if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
	std::vector<uint8_t> v;
	uint8_t buf[65536];
	for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
	fclose(f);
	return v;
}

// the stream from an allocation of exactly its size: an access past it is the sanitizer's to find (std::vector<uint8_t> of that size is one)
static Result run_sort(const std::vector<uint8_t> &in, int32_t n_ref, int64_t seg, bool rev)
{
	Result r;
	const int64_t n = (int64_t)in.size();
	std::vector<uint8_t> s(in.begin(), in.end());
	s.shrink_to_fit();
	r.out.assign((size_t)n, 0xA5);
	SimDrv drv; drv.rev = rev;
	const BsStream t = {s.data(), n, 0, seg, n_ref, 0};
	std::vector<int64_t> segmem((size_t)bs_seg_words(bs_n_seg(t)), 0x5A5A5A5A5A5A5A5Aull);
	BsSegs w; w.carve(segmem.data(), bs_n_seg(t));
	r.status = bs_discover(drv, t, w, &r.f);
	if (r.status != BS_OK) return r;
	r.n_records = r.f.n_records;
	std::vector<int64_t> rec_off((size_t)r.n_records + 1, -7), size((size_t)r.n_records, -7);
	std::vector<uint64_t> k0((size_t)r.n_records), k1((size_t)r.n_records);
	std::vector<uint32_t> v0((size_t)r.n_records), v1((size_t)r.n_records);
	r.rec_off.assign((size_t)r.n_records + 1, -7);
	bs_fill(drv, t, w, r.f, rec_off.data());
	BsSortMem m = {size.data(), r.rec_off.data(), {k0.data(), k1.data()}, {v0.data(), v1.data()}};
	bs_sort_gather(drv, s.data(), rec_off.data(), r.n_records, n_ref, m, r.out.data());
	return r;
}

static Result run_copy(const std::vector<uint8_t> &in, int32_t n_ref, int64_t seg, bool rev, int64_t slab)
{
	Result r;
	const int64_t n = (int64_t)in.size();
	SimDrv drv; drv.rev = rev;
	BsCarry c = {0, 0, 0, 0, 0, 0};
	for (int64_t a = 0; a < n; a += slab) {
		const int64_t b = a + slab < n ? a + slab : n, keep = bs_slab_keep(a);
		std::vector<uint8_t> buf(in.begin() + (a - keep), in.begin() + b);
		buf.shrink_to_fit();
		const BsStream t = {buf.data(), b - a + keep, bs_slab_entry(a, c.exit), seg, n_ref, 1};
		std::vector<int64_t> segmem((size_t)bs_seg_words(bs_n_seg(t)), 0x5A5A5A5A5A5A5A5Aull);
		BsSegs w; w.carve(segmem.data(), bs_n_seg(t));
		if (bs_count_slab(drv, buf.data(), a, b, seg, n_ref, w, c) != BS_OK) { r.status = BS_E_CHAIN; return r; }
	}
	if (c.exit != n) { r.status = BS_E_CHAIN; return r; }
	r.n_records = c.n_records;
	r.f = BsFound{c.n_records, c.exit, c.n_seg, c.right, c.repaired, c.rounds};
	return r;
}

int main(int argc, char **argv)
{
	if (argc >= 5 && !strcmp(argv[1], "time")) {
		const std::vector<uint8_t> in = slurp(argv[2]);
		const auto t0 = std::chrono::steady_clock::now();
		const Result r = run_sort(in, atoi(argv[3]), atoll(argv[4]), false);
		const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		printf("status %d\nrecords %lld\nms %.3f\n", r.status, (long long)r.n_records, ms);
		return 0;
	}
	const bool copy = argc >= 6 && !strcmp(argv[1], "copy");
	if (!copy && !(argc >= 5 && !strcmp(argv[1], "sort"))) { fprintf(stderr, "usage: bam_sort_sim sort IN OUT N_REF | copy IN OUT N_REF SLAB | time IN N_REF SEG\n"); return 2; }
	const std::vector<uint8_t> in = slurp(argv[2]);
	const int32_t n_ref = atoi(argv[4]);
	const int64_t slab = copy ? atoll(argv[5]) : 0;
	if (copy && slab < 1) return 2;
	Result first;
	std::vector<BsFound> found;
	std::vector<std::pair<int64_t, int> > cfg;
	bool have = false;
	for (int64_t seg : {(int64_t)64, (int64_t)256, (int64_t)4096}) {
		for (int rev = 0; rev < 2; ++rev) {
			Result r = copy ? run_copy(in, n_ref, seg, rev != 0, slab) : run_sort(in, n_ref, seg, rev != 0);
			found.push_back(r.f); cfg.push_back({seg, rev});
			if (!have) { first = std::move(r); have = true; continue; }
			if (r.status != first.status || r.n_records != first.n_records || r.out != first.out || r.rec_off != first.rec_off) {
				fprintf(stderr, "seg %lld rev %d disagrees with the first run (status %d / %d, records %lld / %lld)\n", (long long)seg, rev, r.status, first.status,
				        (long long)r.n_records, (long long)first.n_records);
				return 3;
			}
		}
	}
	if (!copy) {
		FILE *o = fopen(argv[3], "wb");
		if (!o) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
		if (!first.out.empty()) fwrite(first.out.data(), 1, first.out.size(), o);
		fclose(o);
	}
	printf("status %d\nrecords %lld\n", first.status, (long long)first.n_records);
	for (size_t k = 0; k < found.size(); ++k)
		printf("cfg %lld %d %lld %lld %lld %lld\n", (long long)cfg[k].first, cfg[k].second, (long long)found[k].n_seg, (long long)found[k].right, (long long)found[k].repaired,
		       (long long)found[k].rounds);
	printf("rec_off");
	for (int64_t x : first.rec_off) printf(" %lld", (long long)x);
	printf("\n");
	return 0;
}

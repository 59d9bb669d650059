// tests/baisim/bam_index_sim.cpp -- TEST PROGRAM, not part of the product: arachne_amd/csrc/dev_bamindex.h (and with it dev_bamsort.h's
// discovery) compiled for the host, the items of a launch run one after the other in a loop, the run sort by std::stable_sort.
// tests/test_bam_index_sim.py builds it with -fsanitize=address,undefined and runs it as a plain process.
//
//   bam_index_sim CASE OUT SLAB [SLAB ...]
// CASE: little-endian int64 n_bytes, hdr, n_ref, n_blocks; then as int64 ref_len[n_ref], blk_at[n_blocks + 1], blk_isize[n_blocks]; then the
// n_bytes of the inflated stream.  The stream is indexed at every SLAB (inflated bytes of a slab; 0: one slab), at seg_bytes 64, 256 and 4096,
// the items of every launch in ascending and in descending order; every buffer is an allocation of exactly its size.  All runs must agree in
// status, error word and bytes (exit status 3 otherwise).  OUT: the .bai's bytes (not written unless the status is 0).
// Prints "status S" (dev_bamindex.h's BI_*; 4: bad table), "err E" (record << 8 | rule, or -1), then "records", "no_coor", "runs", "chunks",
// "bins", "lin", "slabs" (of the first SLAB) and "configs" with a number each.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "../../arachne_amd/csrc/dev_bamindex.h"

using namespace arx;

struct SimBuf { // exactly the bytes asked for: an access past them is the sanitizer's to find
	void *p = nullptr;
	SimBuf() {}
	SimBuf(const SimBuf &) = delete;
	SimBuf &operator=(const SimBuf &) = delete;
	SimBuf(SimBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
	SimBuf &operator=(SimBuf &&o) noexcept { if (this != &o) { release(); p = o.p; o.p = nullptr; } return *this; }
	void alloc(size_t n) { release(); p = malloc(n ? n : 1); if (!p) abort(); memset(p, 0x5A, n ? n : 1); }
	void release() { free(p); p = nullptr; }
	~SimBuf() { release(); }
	template <class T> T *as() const { return (T *)p; }
};

struct SimDrv {
	typedef SimBuf Buf;
	bool rev = false;
	template <class F> void items(const char *, int64_t n, const F &f)
	{
		if (rev) for (int64_t i = n - 1; i >= 0; --i) f(i);
		else for (int64_t i = 0; i < n; ++i) f(i);
	}
	void scan(const int64_t *in, int64_t *out, int64_t n, const char * = nullptr) { int64_t a = 0; for (int64_t i = 0; i < n; ++i) { out[i] = a; a += in[i]; } out[n] = a; }
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
	void upload(void *d, const void *h, size_t n) { if (n) memcpy(d, h, n); }
	void fetch(void *h, const void *d, size_t n) { if (n) memcpy(h, d, n); }
	void copy(void *d, const void *s, size_t n) { if (n) memcpy(d, s, n); }
	void fill(void *d, int byte, size_t n) { if (n) memset(d, byte, n); }
};

struct SimSrc {
	const uint8_t *stream; const BiBlocks &B;
	bool load(int64_t k, uint8_t *dst, int64_t n) { if (n) memcpy(dst, stream + B.cut_o[(size_t)k], (size_t)n); return true; }
};

struct Result { int status = 0; uint64_t err = BI_UNSET; std::vector<uint8_t> bai; BiIndex ix; };

int main(int argc, char **argv)
{
	if (argc < 4) { fprintf(stderr, "usage: bam_index_sim CASE OUT SLAB [SLAB ...]\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
	std::vector<uint8_t> raw;
	uint8_t chunk[65536];
	for (size_t k; (k = fread(chunk, 1, sizeof chunk, f)) > 0;) raw.insert(raw.end(), chunk, chunk + k);
	fclose(f);
	if (raw.size() < 32) return 2;
	int64_t h4[4];
	memcpy(h4, raw.data(), 32);
	const int64_t n_bytes = h4[0], hdr = h4[1], n_ref = h4[2], n_blocks = h4[3], n_words = 4 + n_ref + 2 * n_blocks + 1;
	if (n_bytes < 0 || n_ref < 0 || n_blocks < 0 || (int64_t)raw.size() != 8 * n_words + n_bytes) { fprintf(stderr, "bad case file\n"); return 2; }
	std::vector<int64_t> words((size_t)n_words);
	memcpy(words.data(), raw.data(), (size_t)n_words * 8);
	std::vector<int32_t> ref_len((size_t)n_ref), isize((size_t)n_blocks);
	for (int64_t i = 0; i < n_ref; ++i) ref_len[(size_t)i] = (int32_t)words[(size_t)(4 + i)];
	const std::vector<int64_t> blk_at(words.begin() + 4 + n_ref, words.begin() + 4 + n_ref + n_blocks + 1);
	for (int64_t b = 0; b < n_blocks; ++b) isize[(size_t)b] = (int32_t)words[(size_t)(4 + n_ref + n_blocks + 1 + b)];
	std::vector<uint8_t> stream(raw.begin() + 8 * n_words, raw.end());
	stream.shrink_to_fit();

	if (bi_long_contig((int32_t)n_ref, ref_len.data()) >= 0) { printf("status 4\n"); return 0; }
	Result first;
	bool have = false;
	int configs = 0;
	int64_t slabs_first = 0;
	for (int a = 3; a < argc; ++a) {
		const int64_t slab = atoll(argv[a]);
		BiBlocks B;
		if (!B.build(n_blocks, blk_at.data(), isize.data(), slab) || B.total != n_bytes) { printf("status 4\n"); return 0; }
		if (a == 3) slabs_first = B.n_slabs();
		for (int64_t seg : {(int64_t)64, (int64_t)256, (int64_t)4096}) {
			for (int rev = 0; rev < 2; ++rev) {
				SimDrv drv; drv.rev = rev != 0;
				SimSrc src{stream.data(), B};
				Result r;
				r.status = bi_run(drv, src, B, hdr, (int32_t)n_ref, ref_len.data(), seg, r.ix);
				r.err = r.ix.err;
				if (r.status == BI_OK) r.bai = bi_serialise(r.ix);
				++configs;
				if (!have) { first = std::move(r); have = true; continue; }
				if (r.status != first.status || r.err != first.err || r.bai != first.bai || (r.status == BI_OK && (r.ix.n_runs != first.ix.n_runs || r.ix.n_records != first.ix.n_records))) {
					fprintf(stderr, "slab %lld seg %lld rev %d disagrees with the first run (status %d / %d, err %lld / %lld, %zu / %zu bytes)\n", (long long)slab, (long long)seg, rev,
					        r.status, first.status, (long long)r.err, (long long)first.err, r.bai.size(), first.bai.size());
					return 3;
				}
			}
		}
	}
	if (first.status == BI_OK) {
		FILE *o = fopen(argv[2], "wb");
		if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
		fwrite(first.bai.data(), 1, first.bai.size(), o);
		fclose(o);
	}
	const BiIndex &x = first.ix;
	printf("status %d\nerr %lld\nrecords %lld\nno_coor %lld\nruns %lld\nchunks %lld\nbins %lld\nlin %lld\nslabs %lld\nconfigs %d\n", first.status, (long long)first.err,
	       (long long)x.n_records, (long long)x.n_no_coor, (long long)x.n_runs, (long long)x.n_chunks, (long long)x.n_bins, (long long)x.n_lin, (long long)slabs_first, configs);
	return 0;
}

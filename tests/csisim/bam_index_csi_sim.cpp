// tests/csisim/bam_index_csi_sim.cpp -- TEST PROGRAM, not part of the product: arachne_amd/csrc/dev_bamindex.h compiled for the host and run
// under the scheme of a CSI index, the items of a launch one after the other in a loop, the run sort by std::stable_sort (the driver is
// tests/baisim/bam_index_sim.cpp's).  tests/test_bam_index_csi_sim.py builds it with -fsanitize=address,undefined and runs it as a plain process.
//
//   bam_index_csi_sim CASE OUT BAI_OUT SLAB [SLAB ...]
// CASE: little-endian int64 n_bytes, hdr, n_ref, n_blocks, min_shift; then as int64 ref_len[n_ref], blk_at[n_blocks + 1], blk_isize[n_blocks];
// then the n_bytes of the inflated stream.  The stream is indexed at every SLAB (inflated bytes of a slab; 0: one slab), at seg_bytes 64, 256
// and 4096, the items of every launch in ascending and in descending order; every buffer is an allocation of exactly its size.  All runs must
// agree in status, error word and bytes (exit status 3 otherwise).  OUT: the .csi's inflated bytes (not written unless the status is 0).
// Where no contig exceeds 2^29 the same configurations are run once more under the BAI's scheme, through the same functors, and BAI_OUT
// receives the .bai's bytes.
// Prints "status S" (dev_bamindex.h's BI_*; 4: bad table or min_shift), "err E" (record << 8 | rule, or -1), then "records", "no_coor", "runs",
// "chunks", "bins", "depth", "min_shift", "slabs" (of the first SLAB), "configs" and "bai_configs" with a number each.
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
		const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1; // as the radix sort: the bits above are not looked at
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

struct Result { int status = 0; uint64_t err = BI_UNSET; std::vector<uint8_t> bytes; BiIndex ix; };
struct Input {
	int64_t n_bytes, hdr, n_blocks; int32_t n_ref;
	std::vector<int32_t> ref_len, isize; std::vector<int64_t> blk_at; std::vector<uint8_t> stream; std::vector<int64_t> slabs;
};

// every configuration under one scheme -> 0, or 3 where two runs disagree, 4 where the table is bad
static int run_all(const Input &in, const BiScheme sc, bool csi, Result &first, int &configs, int64_t &slabs_first)
{
	bool have = false;
	for (size_t a = 0; a < in.slabs.size(); ++a) {
		BiBlocks B;
		if (!B.build(in.n_blocks, in.blk_at.data(), in.isize.data(), in.slabs[a]) || B.total != in.n_bytes) return 4;
		if (a == 0) slabs_first = B.n_slabs();
		for (int64_t seg : {(int64_t)64, (int64_t)256, (int64_t)4096}) {
			for (int rev = 0; rev < 2; ++rev) {
				SimDrv drv; drv.rev = rev != 0;
				SimSrc src{in.stream.data(), B};
				Result r;
				r.status = bi_run(drv, src, B, in.hdr, in.n_ref, in.ref_len.data(), seg, r.ix, sc);
				r.err = r.ix.err;
				if (r.status == BI_OK) r.bytes = csi ? bi_serialise_csi(r.ix) : bi_serialise(r.ix);
				++configs;
				if (!have) { first = std::move(r); have = true; continue; }
				if (r.status != first.status || r.err != first.err || r.bytes != first.bytes || (r.status == BI_OK && (r.ix.n_runs != first.ix.n_runs || r.ix.n_records != first.ix.n_records))) {
					fprintf(stderr, "%s: slab %lld seg %lld rev %d disagrees with the first run (status %d / %d, err %lld / %lld, %zu / %zu bytes)\n", csi ? "csi" : "bai",
					        (long long)in.slabs[a], (long long)seg, rev, r.status, first.status, (long long)r.err, (long long)first.err, r.bytes.size(), first.bytes.size());
					return 3;
				}
			}
		}
	}
	return 0;
}

static bool write_file(const char *path, const std::vector<uint8_t> &v)
{
	FILE *o = fopen(path, "wb");
	if (!o) { fprintf(stderr, "cannot write %s\n", path); return false; }
	fwrite(v.data(), 1, v.size(), o);
	fclose(o);
	return true;
}

int main(int argc, char **argv)
{
	if (argc < 5) { fprintf(stderr, "usage: bam_index_csi_sim CASE OUT BAI_OUT SLAB [SLAB ...]\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
	std::vector<uint8_t> raw;
	uint8_t chunk[65536];
	for (size_t k; (k = fread(chunk, 1, sizeof chunk, f)) > 0;) raw.insert(raw.end(), chunk, chunk + k);
	fclose(f);
	if (raw.size() < 40) return 2;
	int64_t h5[5];
	memcpy(h5, raw.data(), 40);
	Input in;
	in.n_bytes = h5[0]; in.hdr = h5[1]; in.n_ref = (int32_t)h5[2]; in.n_blocks = h5[3];
	const int64_t n_ref = h5[2], min_shift = h5[4], n_words = 5 + n_ref + 2 * in.n_blocks + 1;
	if (in.n_bytes < 0 || n_ref < 0 || n_ref > 1000000 || in.n_blocks < 0 || (int64_t)raw.size() != 8 * n_words + in.n_bytes) { fprintf(stderr, "bad case file\n"); return 2; }
	std::vector<int64_t> words((size_t)n_words);
	memcpy(words.data(), raw.data(), (size_t)n_words * 8);
	in.ref_len.resize((size_t)n_ref); in.isize.resize((size_t)in.n_blocks);
	for (int64_t i = 0; i < n_ref; ++i) in.ref_len[(size_t)i] = (int32_t)words[(size_t)(5 + i)];
	in.blk_at.assign(words.begin() + 5 + n_ref, words.begin() + 5 + n_ref + in.n_blocks + 1);
	for (int64_t b = 0; b < in.n_blocks; ++b) in.isize[(size_t)b] = (int32_t)words[(size_t)(5 + n_ref + in.n_blocks + 1 + b)];
	in.stream.assign(raw.begin() + 8 * n_words, raw.end());
	in.stream.shrink_to_fit();
	for (int a = 4; a < argc; ++a) in.slabs.push_back(atoll(argv[a]));

	const int32_t shift = min_shift < -1000 || min_shift > 1000 ? -1 : bi_csi_shift((int32_t)min_shift);
	if (shift < 0) { printf("status 4\n"); return 0; }
	const BiScheme sc = bi_csi_scheme(shift, in.n_ref, in.ref_len.data());
	Result first, bai;
	int configs = 0, bai_configs = 0;
	int64_t slabs_first = 0, unused = 0;
	int rc = run_all(in, sc, true, first, configs, slabs_first);
	if (rc == 4) { printf("status 4\n"); return 0; }
	if (rc) return rc;
	if (bi_long_contig(in.n_ref, in.ref_len.data()) < 0) {
		rc = run_all(in, BI_BAI, false, bai, bai_configs, unused);
		if (rc) return rc == 4 ? 2 : rc;
		if (bai.status != first.status || bai.err != first.err) { fprintf(stderr, "the two schemes disagree in status or error word\n"); return 3; }
		if (bai.status == BI_OK && !write_file(argv[3], bai.bytes)) return 2;
	}
	if (first.status == BI_OK && !write_file(argv[2], first.bytes)) return 2;
	const BiIndex &x = first.ix;
	printf("status %d\nerr %lld\nrecords %lld\nno_coor %lld\nruns %lld\nchunks %lld\nbins %lld\ndepth %d\nmin_shift %d\nslabs %lld\nconfigs %d\nbai_configs %d\n", first.status,
	       (long long)first.err, (long long)x.n_records, (long long)x.n_no_coor, (long long)x.n_runs, (long long)x.n_chunks, (long long)x.n_bins, (int)sc.depth, (int)sc.min_shift,
	       (long long)slabs_first, configs, bai_configs);
	return 0;
}

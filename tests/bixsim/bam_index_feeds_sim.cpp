// tests/bixsim/bam_index_feeds_sim.cpp -- TEST PROGRAM, not part of the product: the push form of arachne_amd/csrc/dev_bamindex.h (BiPush: the
// index a writer builds of what it is handed) compiled for the host, the items of a launch run one after the other in a loop, the run sort by
// std::stable_sort.  tests/test_bam_index_feeds_sim.py builds it with -fsanitize=address,undefined and runs it as a plain process.
//
//   bam_index_feeds_sim CASE OUT MIN_SHIFT FEEDS PIECE [PIECE ...]
// CASE: the case file of tests/baisim/bam_index_sim.cpp (blk_isize is read and ignored: the layout is the writer's arithmetic, n_blocks must be
// its count).  MIN_SHIFT: -1 for the .bai, else the .csi's (0: 14).  FEEDS: little-endian int64 groups "n_feeds, feed_end[n_feeds]" -- offsets of
// the stream where the feeds end, the last being n_bytes; the feeds of a group are the record stream behind the header cut there.  The stream is
// indexed under every group at every PIECE (bytes of a feed indexed at once; 0: the whole feed), at seg_bytes 64, 256 and 4096, the items of every
// launch in ascending and in descending order; every buffer is an allocation of exactly its size and every feed a copy of exactly its bytes.
// All runs must agree in status, error word and bytes (exit status 3 otherwise).  OUT: the index's bytes (the .csi's inflated), not written
// unless the status is 0.  Prints "status S" (BI_*; 4: bad table or contigs), "err E", "records", "no_coor", "runs", "configs" with a number each.
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

struct Result { int status = 0; uint64_t err = BI_UNSET; std::vector<uint8_t> out; int64_t n_records = 0, n_no_coor = 0, n_runs = 0; };

static std::vector<uint8_t> slurp(const char *path)
{
	std::vector<uint8_t> raw;
	FILE *f = fopen(path, "rb");
	if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
	uint8_t chunk[65536];
	for (size_t k; (k = fread(chunk, 1, sizeof chunk, f)) > 0;) raw.insert(raw.end(), chunk, chunk + k);
	fclose(f);
	return raw;
}

int main(int argc, char **argv)
{
	if (argc < 6) { fprintf(stderr, "usage: bam_index_feeds_sim CASE OUT MIN_SHIFT FEEDS PIECE [PIECE ...]\n"); return 2; }
	const std::vector<uint8_t> raw = slurp(argv[1]);
	if (raw.size() < 32) return 2;
	int64_t h4[4];
	memcpy(h4, raw.data(), 32);
	const int64_t n_bytes = h4[0], hdr = h4[1], n_ref = h4[2], n_blocks = h4[3], n_words = 4 + n_ref + 2 * n_blocks + 1;
	if (n_bytes < 0 || hdr < 0 || hdr > n_bytes || n_ref < 0 || n_blocks < 0 || (int64_t)raw.size() != 8 * n_words + n_bytes) { fprintf(stderr, "bad case file\n"); return 2; }
	std::vector<int64_t> words((size_t)n_words);
	memcpy(words.data(), raw.data(), (size_t)n_words * 8);
	std::vector<int32_t> ref_len((size_t)n_ref);
	for (int64_t i = 0; i < n_ref; ++i) ref_len[(size_t)i] = (int32_t)words[(size_t)(4 + i)];
	const std::vector<int64_t> blk_at(words.begin() + 4 + n_ref, words.begin() + 4 + n_ref + n_blocks + 1);
	const int min_shift = atoi(argv[3]);
	const bool csi = min_shift >= 0;
	const int32_t shift = csi ? bi_csi_shift(min_shift) : 0;
	const std::vector<uint8_t> fraw = slurp(argv[4]);
	std::vector<int64_t> fw(fraw.size() / 8);
	memcpy(fw.data(), fraw.data(), fw.size() * 8);

	const int64_t layout = bi_header_blocks(hdr) + (n_bytes - hdr + BI_BLOCK - 1) / BI_BLOCK;
	bool bad = shift < 0 || layout != n_blocks || (!csi && bi_long_contig((int32_t)n_ref, ref_len.data()) >= 0);
	for (int64_t b = 0; b <= n_blocks && !bad; ++b) bad = blk_at[(size_t)b] < 0 || blk_at[(size_t)b] >= BI_MAX_AT || (b > 0 && blk_at[(size_t)b] <= blk_at[(size_t)b - 1]);
	if (bad) { printf("status 4\n"); return 0; }
	const BiScheme sc = csi ? bi_csi_scheme(shift, (int32_t)n_ref, ref_len.data()) : BI_BAI;

	Result first;
	bool have = false;
	int configs = 0;
	for (size_t g = 0; g < fw.size();) {
		const int64_t n_feeds = fw[g];
		if (n_feeds < 1 || g + 1 + (size_t)n_feeds > fw.size() || fw[g + (size_t)n_feeds] != n_bytes) { fprintf(stderr, "bad feeds file\n"); return 2; }
		const int64_t *feed_end = &fw[g + 1];
		for (int a = 5; a < argc; ++a) {
			const int64_t piece = atoll(argv[a]);
			for (int64_t seg : {(int64_t)64, (int64_t)256, (int64_t)4096}) {
				for (int rev = 0; rev < 2; ++rev) {
					SimDrv drv; drv.rev = rev != 0;
					BiPush<SimDrv> push;
					push.begin(drv, (int32_t)n_ref, ref_len.data(), sc, hdr, seg, piece);
					Result r;
					int64_t at = hdr;
					for (int64_t k = 0; k < n_feeds && r.status == BI_OK; ++k) {
						const int64_t e = feed_end[k];
						if (e < at || e > n_bytes) { if (e < hdr) continue; fprintf(stderr, "bad feeds file\n"); return 2; }
						std::vector<uint8_t> bytes(raw.begin() + 8 * n_words + at, raw.begin() + 8 * n_words + e); // a copy of exactly the feed
						bytes.shrink_to_fit();
						r.status = push.feed(drv, bytes.data(), e - at);
						at = e;
					}
					if (r.status == BI_OK) r.status = push.finish(drv, blk_at.data());
					r.err = push.ix.err; r.n_records = push.ix.n_records; r.n_no_coor = push.ix.n_no_coor; r.n_runs = push.ix.n_runs;
					if (r.status == BI_OK) r.out = csi ? bi_serialise_csi(push.ix) : bi_serialise(push.ix);
					++configs;
					if (!have) { first = std::move(r); have = true; continue; }
					if (r.status != first.status || r.err != first.err || r.out != first.out || (r.status == BI_OK && (r.n_runs != first.n_runs || r.n_records != first.n_records))) {
						fprintf(stderr, "feeds %lld piece %lld seg %lld rev %d disagrees with the first run (status %d / %d, err %lld / %lld, %zu / %zu bytes)\n", (long long)n_feeds,
						        (long long)piece, (long long)seg, rev, r.status, first.status, (long long)r.err, (long long)first.err, r.out.size(), first.out.size());
						return 3;
					}
				}
			}
		}
		g += 1 + (size_t)n_feeds;
	}
	if (first.status == BI_OK) {
		FILE *o = fopen(argv[2], "wb");
		if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
		fwrite(first.out.data(), 1, first.out.size(), o);
		fclose(o);
	}
	printf("status %d\nerr %lld\nrecords %lld\nno_coor %lld\nruns %lld\nconfigs %d\n", first.status, (long long)first.err, (long long)first.n_records, (long long)first.n_no_coor,
	       (long long)first.n_runs, configs);
	return 0;
}

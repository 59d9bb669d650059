// tests/bgzfsim/bgzf_sim.cpp -- TEST PROGRAM, not part of the product: arachne_amd/csrc/dev_bgzf.h compiled for the host, the lanes of a
// workgroup run one after the other in a loop and a phase's barrier is the end of that loop.  tests/test_bgzf_sim.py builds it with
// -fsanitize=address,undefined and runs it as a plain process.
//
//   bgzf_sim deflate IN OUT [rev]   IN cut every 65280 bytes, every block through bgzf_block, framed as BamSink::deflate_block frames a block; prints
//                                   "blocks stored fixed dynamic".  rev: the lanes run in descending order (the bytes must not change)
//   bgzf_sim code LIMIT N f0 f1 ..  the code builder on a count vector of N symbols: prints the N lengths
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../arachne_amd/csrc/dev_bgzf.h"

using namespace arx;

struct SimDrv {
	bool rev = false;
	template <class F> void lanes(F f)
	{
		if (rev) for (int l = BGZF_LANES - 1; l >= 0; --l) f(l);
		else for (int l = 0; l < BGZF_LANES; ++l) f(l);
	}
	void scan(const int32_t *in, int32_t *out, int n)
	{
		int run = 0;
		for (int i = 0; i < n; ++i) { out[i] = run; run += in[i]; }
		out[n] = run;
	}
};

static int run_deflate(const char *in_path, const char *out_path, bool rev)
{
	FILE *f = fopen(in_path, "rb");
	if (!f) { fprintf(stderr, "cannot read %s\n", in_path); return 2; }
	std::vector<uint8_t> src;
	uint8_t buf[65536];
	for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) src.insert(src.end(), buf, buf + k);
	fclose(f);
	// exactly the sizes the kernel has: an access past any of them is the sanitizer's to find
	std::vector<uint32_t> mem((BGZF_WORK_BYTES + 3) / 4);
	std::vector<uint16_t> tok(BGZF_IN + 2);
	BgzfWork w;
	bgzf_carve(w, (uint8_t *)mem.data(), tok.data());
	SimDrv drv; drv.rev = rev;
	drv.lanes([&](int lane) { bgzf_tables(w, lane); });
	drv.lanes([&](int lane) { bgzf_shift_table(w, lane); });
	FILE *o = fopen(out_path, "wb");
	if (!o) { fprintf(stderr, "cannot write %s\n", out_path); return 2; }
	long forms[3] = {0, 0, 0}, blocks = 0;
	for (size_t b0 = 0; b0 < src.size(); b0 += BGZF_IN, ++blocks) {
		const int n = src.size() - b0 < (size_t)BGZF_IN ? (int)(src.size() - b0) : BGZF_IN;
		std::vector<uint8_t> blk(src.begin() + b0, src.begin() + b0 + n); // its own allocation: reads past the block are caught
		std::vector<uint32_t> out((BGZF_OUT_SLICE - 26) / 4, 0xA5A5A5A5u); // the slice the issue allows, dirty: the kernel zeroes what it ors into
		uint32_t meta[4];
		bgzf_block(drv, w, blk.data(), n, out.data(), meta);
		if (meta[2] > 2 || meta[3] != (uint32_t)n || meta[0] > 5u + (uint32_t)n) { fprintf(stderr, "bad meta\n"); return 3; }
		++forms[meta[2]];
		const uint32_t clen = meta[0], bsize = 18 + clen + 8 - 1;
		const uint8_t hdr[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8)};
		uint8_t tr[8];
		for (int k = 0; k < 4; ++k) { tr[k] = (uint8_t)(meta[1] >> (8 * k)); tr[4 + k] = (uint8_t)((uint32_t)n >> (8 * k)); }
		fwrite(hdr, 1, 18, o); fwrite(out.data(), 1, clen, o); fwrite(tr, 1, 8, o);
	}
	fclose(o);
	printf("%ld %ld %ld %ld\n", blocks, forms[0], forms[1], forms[2]);
	return 0;
}

static int run_code(int argc, char **argv)
{
	const int limit = atoi(argv[2]), n = atoi(argv[3]);
	if (n < 1 || n > BGZF_LL || argc != 4 + n || (limit != 15 && limit != 7)) { fprintf(stderr, "usage: bgzf_sim code LIMIT N f0 .. f(N-1)\n"); return 2; }
	std::vector<uint32_t> freq(n), tree(n);
	std::vector<uint16_t> order(n), code(n);
	std::vector<uint8_t> len(n);
	std::vector<int32_t> cnt(64);
	for (int i = 0; i < n; ++i) freq[i] = (uint32_t)strtoul(argv[4 + i], nullptr, 10);
	for (int lane = 0; lane < BGZF_LANES; ++lane) bgzf_rank(freq.data(), n, order.data(), lane);
	bgzf_build_code(freq.data(), n, order.data(), limit, tree.data(), cnt.data(), len.data(), code.data());
	// the codes must be the canonical ones of the lengths: prefix-free by construction, checked here bit by bit
	for (int a = 0; a < n; ++a)
		for (int b = 0; b < n; ++b)
			if (a != b && len[a] && len[b] && len[a] <= len[b] && (code[b] & ((1u << len[a]) - 1)) == code[a]) { fprintf(stderr, "code %d is a prefix of code %d\n", a, b); return 3; }
	for (int i = 0; i < n; ++i) printf("%d%c", len[i], i + 1 < n ? ' ' : '\n');
	return 0;
}

int main(int argc, char **argv)
{
	if (argc >= 4 && !strcmp(argv[1], "deflate")) return run_deflate(argv[2], argv[3], argc > 4 && !strcmp(argv[4], "rev"));
	if (argc >= 5 && !strcmp(argv[1], "code")) return run_code(argc, argv);
	fprintf(stderr, "usage: bgzf_sim deflate IN OUT [rev] | bgzf_sim code LIMIT N f0 ..\n");
	return 2;
}

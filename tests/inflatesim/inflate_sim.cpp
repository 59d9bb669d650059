// tests/inflatesim/inflate_sim.cpp -- TEST PROGRAM, not part of the product: arachne_amd/csrc/dev_inflate.h compiled for the host, the lanes of
// a wavefront run one after the other in a loop and a phase's hand-off is the end of that loop.  tests/test_inflate_sim.py builds it with
// -fsanitize=address,undefined and runs it as a plain process.
//
//   inflate_sim inflate IN OUT [rev]   IN: a chain of whole BGZF blocks, walked with the product's bgzf_walk; every block through inf_block
//                                      from an allocation of exactly its compressed bytes into one of exactly ISIZE bytes.  OUT: the blocks'
//                                      bytes in order (a bad block's are 0xA5).  Prints "blocks compressed inflated deflate_blocks" and the
//                                      statuses; exit status 4 where the headers do not tile IN.  rev: the lanes run in descending order.
// Every block that is INF_OK is inflated by zlib as well and compared here, apart from the comparison the Python side makes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <zlib.h>
#include "../../arachne_amd/csrc/dev_inflate.h"

using namespace arx;

struct SimDrv {
	bool rev = false;
	template <class F> void lanes(F f)
	{
		if (rev) for (int l = INF_LANES - 1; l >= 0; --l) f(l);
		else for (int l = 0; l < INF_LANES; ++l) f(l);
	}
};

static bool zlib_agrees(const uint8_t *src, int clen, const uint8_t *want, int n)
{
	std::vector<uint8_t> out((size_t)n + 1);
	z_stream z;
	memset(&z, 0, sizeof z);
	if (inflateInit2(&z, -15) != Z_OK) return false;
	z.next_in = (Bytef *)src; z.avail_in = (uInt)clen; z.next_out = out.data(); z.avail_out = (uInt)out.size();
	const int r = inflate(&z, Z_FINISH);
	const bool ok = r == Z_STREAM_END && z.total_out == (uLong)n && (n == 0 || !memcmp(out.data(), want, (size_t)n));
	inflateEnd(&z);
	return ok;
}

int main(int argc, char **argv)
{
	if (argc < 4 || strcmp(argv[1], "inflate")) { fprintf(stderr, "usage: inflate_sim inflate IN OUT [rev]\n"); return 2; }
	FILE *f = fopen(argv[2], "rb");
	if (!f) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
	std::vector<uint8_t> src;
	uint8_t buf[65536];
	for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) src.insert(src.end(), buf, buf + k);
	fclose(f);
	int64_t total = 0;
	const int64_t nb = bgzf_walk(src.data(), (int64_t)src.size(), nullptr, 0, &total);
	if (nb < 0) { printf("untiled\n"); return 4; }
	std::vector<InfRow> rows((size_t)nb);
	bgzf_walk(src.data(), (int64_t)src.size(), rows.data(), nb, &total);
	// exactly the sizes the kernel has: an access past any of them is the sanitizer's to find
	std::vector<uint32_t> mem((INF_WORK_BYTES + 3) / 4);
	std::vector<uint8_t> lds_out(INF_MAX_OUT);
	InfWork w;
	inf_carve(w, (uint8_t *)mem.data(), lds_out.data());
	SimDrv drv; drv.rev = argc > 4 && !strcmp(argv[4], "rev");
	std::vector<uint8_t> all((size_t)total, 0xA5);
	std::vector<int> status((size_t)nb);
	long n_deflate = 0;
	for (int64_t b = 0; b < nb; ++b) {
		const InfRow &r = rows[(size_t)b];
		const int clen = r.clen < 0 ? 0 : r.clen;
		std::vector<uint8_t> in(src.begin() + r.coff, src.begin() + r.coff + clen), dst((size_t)r.isize, 0xA5);
		memset(mem.data(), 0x5A, mem.size() * 4); // dirty work memory: nothing may depend on what the block before left
		int nd = 0;
		status[(size_t)b] = inf_block(drv, w, in.data(), r.clen, r.isize, r.crc, dst.data(), &nd);
		n_deflate += nd;
		if (status[(size_t)b] == INF_OK) {
			if (!zlib_agrees(in.data(), clen, dst.data(), r.isize)) { fprintf(stderr, "block %ld: zlib disagrees\n", (long)b); return 3; }
			if (r.isize) memcpy(all.data() + r.ooff, dst.data(), (size_t)r.isize);
		}
	}
	FILE *o = fopen(argv[3], "wb");
	if (!o) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
	if (!all.empty()) fwrite(all.data(), 1, all.size(), o);
	fclose(o);
	printf("%ld %ld %ld %ld\n", (long)nb, (long)src.size(), (long)total, n_deflate);
	for (int64_t b = 0; b < nb; ++b) printf("%d%c", status[(size_t)b], b + 1 < nb ? ' ' : '\n');
	return 0;
}

// tests/gzfindsim/gzfind_sim.cpp -- TEST PROGRAM, not part of the product: the two forms of the search for block starts of
// arachne_amd/csrc/dev_gunzip.h compiled for the host, the lanes of the wavefront in a loop.  gz_find is the stated reference form (64 positions a
// round); gz_find_runs is what gz_chunk_find calls (a run of positions per lane behind a prefilter).  tests/test_gunzip_find_sim.py builds this
// with -fsanitize=address,undefined and runs it as a plain process.
//
//   gzfind_sim IN CHUNK [rev]   IN: any file; its bytes are the stream.  For every chunk k of CHUNK bytes both forms search the chunk's range
//                               [8 * k * CHUNK, 8 * (k + 1) * CHUNK) of bit positions, each on work memory that was dirtied first.  Prints per
//                               chunk "k cand pre cheap": the position found (-1: none), and how many positions of the range in front of it pass
//                               the prefilter's 13 bits and gz_cheap.  Exit status 3 where the two forms differ on any chunk.  rev: lanes run
//                               in descending order.
// The stream is an allocation of exactly the file's bytes: a read past it is the sanitizer's to find.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../arachne_amd/csrc/dev_gunzip.h"

using namespace arx;

struct SimDrv {
	bool rev = false;
	template <class F> void lanes(F f)
	{
		if (rev) for (int l = INF_LANES - 1; l >= 0; --l) f(l);
		else for (int l = 0; l < INF_LANES; ++l) f(l);
	}
};

int main(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: gzfind_sim IN CHUNK [rev]\n"); return 2; }
	FILE *fp = fopen(argv[1], "rb");
	if (!fp) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
	std::vector<uint8_t> in;
	uint8_t b[65536];
	for (size_t k; (k = fread(b, 1, sizeof b, fp)) > 0;) in.insert(in.end(), b, b + k);
	fclose(fp);
	const int64_t chunk = atoll(argv[2]);
	if (chunk < 64 || in.empty() || (int64_t)in.size() > GZ_MAX_SLAB) { fprintf(stderr, "sizes outside their bounds\n"); return 2; }
	const std::vector<uint8_t> src(in); // exactly the file's bytes
	const int clen = (int)src.size();
	SimDrv drv; drv.rev = argc > 3 && !strcmp(argv[3], "rev");
	std::vector<uint32_t> mem(GZ_FIND_BYTES / 4 + 4); // what the find kernel is given: no ring of symbols behind it
	uint8_t *base = (uint8_t *)mem.data();
	base += (16 - ((uintptr_t)base & 15)) & 15;
	GzWork w;
	gz_carve(w, base);
	int bad = 0;
	const int n = (int)((clen + chunk - 1) / chunk);
	for (int k = 0; k < n; ++k) {
		const int64_t lo = 8 * (int64_t)k * chunk, hi = lo + 8 * chunk < 8 * (int64_t)clen ? lo + 8 * chunk : 8 * (int64_t)clen;
		memset(base, 0x5A, GZ_FIND_BYTES);
		const int want = gz_find(drv, w, src.data(), clen, (int)lo, (int)hi);
		memset(base, 0xA5, GZ_FIND_BYTES);
		const int got = gz_find_runs(drv, w, src.data(), clen, (int)lo, (int)hi);
		if (got != want) { fprintf(stderr, "chunk %d [%lld, %lld): gz_find %d, gz_find_runs %d\n", k, (long long)lo, (long long)hi, want, got); ++bad; }
		// the counts in front of the position found, piece by piece as the searches see the ring
		long pre = 0, cheap = 0;
		const int64_t end = want < 0 ? hi : want;
		for (int64_t piece = lo; piece < end; piece += 8 * GZ_PIECE) {
			drv.lanes([&](int lane) { if (lane == 0) { w.inf.sh[IS_BITPOS] = (int32_t)piece; w.inf.sh[IS_HI] = 0; } });
			drv.lanes([&](int lane) { inf_fill(w.inf, src.data(), clen, lane); });
			for (int64_t p = piece; p < piece + 8 * GZ_PIECE && p < end; ++p) {
				InfBits r;
				r.begin(w.inf.ring, (int)p);
				const bool first13 = r.get(3) == 4u && r.get(5) <= 29u && r.get(5) <= 29u;
				pre += first13;
				const bool ch = gz_cheap(w.inf.ring, (int)p, clen);
				if (ch && !first13) { fprintf(stderr, "position %lld passes gz_cheap and not the prefilter's fields\n", (long long)p); ++bad; }
				cheap += ch;
			}
		}
		printf("%d %d %ld %ld\n", k, want, pre, cheap);
	}
	return bad ? 3 : 0;
}

// tests/hostsim/ext_two_symbol.cpp -- TEST CODE, not part of the product: dev_fm.h compiled for the host on its own, with a main of its own
// (tests/test_ext_two_symbol_hostsim.py builds it with -fsanitize=address,undefined and runs it).
//
// ext_finish<true> (what k_seed_bwd_g<true> runs) counts two symbols at each end of the interval and takes the child's position on the other
// strand from the identity written beside it; extend1() counts all four.  Here: the Occ blocks of a random text and its reverse complement
// (naive suffix sort, the primary row inside, re-packed by occ_repack_block), every bi-interval reached from the empty string by up to 8
// extensions in either direction, every c = 0..3 and both directions on each: all four fields equal, and s_0 + s_1 + s_2 + s_3 = ik.s - cond.
// The program fails unless it met every edge it is there for (the list at the end of main).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <set>
#include <tuple>
#include <vector>
#include "../../arachne_amd/csrc/arx_dev.h"
#include "../../arachne_amd/csrc/dev_fm.h"

using namespace arx;

struct Seen { long n = 0, with_primary = 0, row_minus1 = 0, s1 = 0, one_block = 0, two_blocks = 0; bool off[128] = {}; };

static bool same(const Biv &a, const Biv &b) { return a.k == b.k && a.l == b.l && a.s == b.s && a.info == b.info; }

static int check_interval(const IndexView &ix, const Biv &ik, Seen &sn, Biv kids[2][4])
{
	for (int back = 0; back < 2; ++back) {
		const uint64_t a = back ? ik.k : ik.l;
		const uint64_t cond = a <= ix.primary && a + ik.s - 1 >= ix.primary;
		ExtLoad L;
		ext_issue(ix, ik, back, true, L);
		uint64_t sum = 0;
		for (int c = 0; c < 4; ++c) {
			const Biv two = ext_finish<true>(ix, ik, back, c, L), four = extend1(ix, ik, back, c), gen = ext_finish<false>(ix, ik, back, c, L);
			if (!same(two, four) || !same(gen, four)) {
				fprintf(stderr, "mismatch: ik (%llu %llu %llu) back %d c %d: two-symbol (%llu %llu %llu) extend1 (%llu %llu %llu)\n", (unsigned long long)ik.k, (unsigned long long)ik.l,
				        (unsigned long long)ik.s, back, c, (unsigned long long)two.k, (unsigned long long)two.l, (unsigned long long)two.s, (unsigned long long)four.k, (unsigned long long)four.l, (unsigned long long)four.s);
				return 1;
			}
			sum += four.s;
			kids[back][c] = four;
			++sn.n;
		}
		if (sum != ik.s - cond) { fprintf(stderr, "identity: ik (%llu %llu %llu) back %d: sum %llu, cond %d\n", (unsigned long long)ik.k, (unsigned long long)ik.l, (unsigned long long)ik.s, back, (unsigned long long)sum, (int)cond); return 1; }
		sn.with_primary += (long)(cond && a != 0); // (the empty string's interval holds every row: not counted)
		sn.row_minus1 += a == 0;
		sn.s1 += ik.s == 1;
		if (L.nk) sn.off[L.nk - 1] = true;
		if (L.nl) sn.off[L.nl - 1] = true;
		if (L.nk && L.nl) { // both rows real: the blocks they fall into, as ext_issue computes them
			uint64_t k = a - 1, l = a - 1 + ik.s;
			k -= (k >= ix.primary); l -= (l >= ix.primary);
			if ((k >> 7) == (l >> 7)) ++sn.one_block; else ++sn.two_blocks;
		}
	}
	return 0;
}

int main(int argc, char **argv)
{
	const int half = argc > 1 ? atoi(argv[1]) : 1500;
	uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(argc > 2 ? atoi(argv[2]) + 11 : 11);
	auto rnd = [&](int m) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (int)(x % (uint64_t)m); };
	// the text: a random strand and its reverse complement, as `bwa index` lays a genome out
	const int N = 2 * half;
	std::vector<uint8_t> T((size_t)N);
	for (int i = 0; i < half; ++i) T[(size_t)i] = (uint8_t)rnd(4);
	for (int i = 0; i < half; ++i) T[(size_t)(N - 1 - i)] = (uint8_t)(3 - T[(size_t)i]);
	// suffix array of T$ by a naive sort ($ below every symbol: row 0 is the empty suffix)
	std::vector<int> sa((size_t)N + 1);
	for (int i = 0; i <= N; ++i) sa[(size_t)i] = i;
	std::sort(sa.begin(), sa.end(), [&](int p, int q) {
		while (p < N && q < N) { if (T[(size_t)p] != T[(size_t)q]) return T[(size_t)p] < T[(size_t)q]; ++p; ++q; }
		return p > q; // the one that ran out is the shorter suffix
	});
	// the BWT with the $ taken out, its row remembered (bwt.c: primary)
	std::vector<uint8_t> B;
	uint64_t primary = 0;
	for (int i = 0; i <= N; ++i) { if (sa[(size_t)i] == 0) primary = (uint64_t)i; else B.push_back(T[(size_t)sa[(size_t)i] - 1]); }
	if ((int)B.size() != N) { fprintf(stderr, "bwt length\n"); return 1; }
	// BWA's blocks (per 128 symbols: 4 x u64 counts before the block, 8 x u32 of 16 symbols, most significant first), then the re-packing
	const int n_blk = N / 128 + 2;
	std::vector<uint32_t> blocks((size_t)n_blk * 16, 0);
	uint64_t cum[4] = {0, 0, 0, 0};
	for (int bi = 0; bi < n_blk; ++bi) {
		uint32_t *blk = blocks.data() + (size_t)bi * 16;
		for (int c = 0; c < 4; ++c) { blk[2 * c] = (uint32_t)cum[c]; blk[2 * c + 1] = (uint32_t)(cum[c] >> 32); }
		for (int j = 0; j < 128; ++j) {
			const int p = bi * 128 + j;
			if (p >= N) break;
			blk[8 + (j >> 4)] |= (uint32_t)B[(size_t)p] << (30 - 2 * (j & 15));
			++cum[B[(size_t)p]];
		}
		occ_repack_block(blk);
	}
	IndexView ix = IndexView();
	ix.bwt = blocks.data(); ix.primary = primary; ix.seq_len = (uint64_t)N;
	ix.L2[0] = 0;
	for (int c = 0; c < 4; ++c) ix.L2[c + 1] = ix.L2[c] + cum[c];
	if (!occ_counts_fit32(ix)) { fprintf(stderr, "the text does not qualify for the 32-bit form\n"); return 1; }

	// every bi-interval within 8 extensions of the empty string (k = l = 0, s = N + 1: its lower row is -1), each visited once
	Seen sn;
	std::set<std::tuple<uint64_t, uint64_t, uint64_t>> seen;
	std::vector<Biv> level, next;
	Biv root = Biv(); root.k = 0; root.l = 0; root.s = (uint64_t)N + 1; root.info = 0;
	level.push_back(root);
	for (int depth = 0; depth <= 8 && !level.empty(); ++depth) {
		next.clear();
		for (const Biv &ik : level) {
			Biv kids[2][4];
			if (check_interval(ix, ik, sn, kids)) return 1;
			if (depth == 8) continue;
			for (int back = 0; back < 2; ++back)
				for (int c = 0; c < 4; ++c) {
					const Biv &kid = kids[back][c];
					if (kid.s > 0 && seen.insert(std::make_tuple(kid.k, kid.l, kid.s)).second) next.push_back(kid);
				}
		}
		level.swap(next);
	}
	printf("extensions %ld intervals %zu with_primary %ld row_minus1 %ld s1 %ld one_block %ld two_blocks %ld off0 %d off31 %d off32 %d off127 %d primary %llu\n", sn.n, seen.size() + 1,
	       sn.with_primary, sn.row_minus1, sn.s1, sn.one_block, sn.two_blocks, (int)sn.off[0], (int)sn.off[31], (int)sn.off[32], (int)sn.off[127], (unsigned long long)primary);
	// the edges this program is there for
	if (!sn.with_primary) { fprintf(stderr, "no interval contained the primary row\n"); return 2; }
	if (!sn.row_minus1) { fprintf(stderr, "no interval had the row -1 below it\n"); return 2; }
	if (!sn.s1) { fprintf(stderr, "no interval of one row\n"); return 2; }
	if (!sn.off[0] || !sn.off[127] || !sn.off[31] || !sn.off[32]) { fprintf(stderr, "a block or quarter edge was not met\n"); return 2; }
	if (!sn.one_block || !sn.two_blocks) { fprintf(stderr, "both ends in one block and in two: one of them was not met\n"); return 2; }
	return 0;
}

// tests/hostsim/ext_closed.cpp -- TEST CODE, not part of the product: dev_sw.h compiled for the host on its own, for the unit test of the
// extensions their diagonal decides (tests/test_ext_closed_hostsim.py builds it into a small library of its own and calls the entry below).
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../arachne_amd/csrc/arx_dev.h"
#include "../../arachne_amd/csrc/dev_sw.h"

// test entry: the extensions their diagonal decides (dev_sw.h ext_closed_form) against ext2_task on the same task, all six fields, and the
// word-wise walk against the pair-by-pair one.  A grid first -- qlen 1 .. 12 and longer queries up to 255, no differing pair and the single one
// at every position (the longer ones: the first and last eight and a few between), two differing pairs, a base of 4 in the read; h0 of 4, 5, 19
// and 150; tlen of qlen - 1, qlen, qlen + 1 and qlen + 200; both directions, both strands, windows at the low end, the high end and inside
// their strand (so position 0, l_pac and 2 * l_pac are all touched) -- then `iters` random tasks, directions of read and reference drawn apart.
// out[0]: tasks; [1]: tasks that had to be accepted by construction; [2]: accepted; [3]: accepted or declined against the construction;
// [4]: accepted with a field that differs from ext2_task's; [5]: word-wise and pair-by-pair forms differ.  Returns out[0].
extern "C" long arx_test_ext_closed(unsigned seed, int iters, long *out)
{
	using namespace arx;
	uint64_t x = 0x9E3779B97F4A7C15ull * (seed + 11);
	auto rnd = [&](int m) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (int)(x % (uint64_t)m); };
	for (int i = 0; i < 6; ++i) out[i] = 0;
	std::vector<uint8_t> store; IndexView ix = IndexView();
	auto new_strand = [&]() {
		const int64_t l_pac = 520 + rnd(300);
		store.assign((size_t)(l_pac / 4 + 1), 0); // no spare bytes behind the strand: a read past its last byte shows under a sanitizer
		for (int64_t p = 0; p < l_pac; ++p) store[p >> 2] |= (uint8_t)(rnd(4) << ((~p & 3) << 1));
		ix.pac = store.data(); ix.l_pac = l_pac; ix.seq_len = (uint64_t)(2 * l_pac);
	};
	std::vector<uint32_t> row(MAX_READ_LEN + 2);
	// mm1, mm2: indices of differing pairs (-1: none); amb: index of a base of 4 (-1: none); edge 0 / 1 / 2: low end, high end, inside
	auto one = [&](int qlen, int tlen, int h0, int qdir, int tdir, bool rev, int edge, int mm1, int mm2, int amb, int w) {
		const int64_t L = ix.l_pac, lo = (rev ? L : 0) + (edge == 0 ? 0 : edge == 1 ? L - tlen : rnd((int)(L - tlen + 1)));
		std::vector<uint8_t> q((size_t)qlen + 11, 9);
		ExtTask t;
		t.owner = 0; t.qlen = qlen; t.tlen = tlen; t.qdir = qdir; t.tdir = tdir; t.w = w; t.h0 = h0;
		t.tpos = tdir > 0 ? lo : lo + tlen - 1;
		t.qoff = rnd(4) + (qdir > 0 ? 0 : qlen - 1);
		for (int j = 0; j < qlen; ++j) {
			int b = j < tlen ? ref_base(ix, t.tpos + (int64_t)j * tdir) : rnd(4);
			if (j == mm1 || j == mm2) b = (b + 1 + rnd(3)) & 3;
			if (j == amb) b = 4;
			q[(size_t)(t.qoff + j * qdir)] = (uint8_t)b;
		}
		const int n_mm = (mm1 >= 0 && mm1 < qlen) + (mm2 >= 0 && mm2 < qlen && mm2 != mm1);
		const bool want = qlen > 0 && tlen >= qlen && h0 >= 5 && !(amb >= 0 && amb < qlen) && n_mm <= 1;
		ExtRes a = ExtRes(), b = ExtRes();
		const bool got = ext_closed_form(ix, q.data(), t, a), got_p = ext_closed_form_pairwise(ix, q.data(), t, b);
		++out[0]; out[1] += want; out[2] += got; out[3] += got != want;
		if (got != got_p || (got && memcmp(&a, &b, sizeof(ExtRes)))) ++out[5];
		if (got) {
			const ExtRes e = ext2_task(ix, q.data(), t, row.data(), 1);
			if (e.score != a.score || e.qle != a.qle || e.tle != a.tle || e.gtle != a.gtle || e.gscore != a.gscore || e.max_off != a.max_off) ++out[4];
		}
	};
	static const int long_q[] = {13, 16, 17, 31, 64, 100, 149, 150, 254, 255}, h0s[] = {4, 5, 19, 150};
	for (int qi = 0; qi < 22; ++qi) {
		const int qlen = qi < 12 ? qi + 1 : long_q[qi - 12];
		new_strand();
		std::vector<int> mm; // -1: none; the single differing pair's index otherwise
		mm.push_back(-1);
		for (int p = 0; p < qlen; ++p) if (qlen <= 12 || p < 8 || p >= qlen - 8 || p % 37 == 5) mm.push_back(p);
		for (int hi = 0; hi < 4; ++hi) for (int ti = 0; ti < 4; ++ti) {
			const int h0 = h0s[hi], tlen = ti == 0 ? qlen - 1 : ti == 1 ? qlen : ti == 2 ? qlen + 1 : qlen + 200;
			for (int dir = -1; dir <= 1; dir += 2) for (int rev = 0; rev < 2; ++rev) for (int edge = 0; edge < 3; ++edge) {
				if (qlen > 12 && edge != (hi + ti + rev + (dir > 0)) % 3) continue; // the longer ones: one placement per combination, all three met
				for (size_t k = 0; k < mm.size(); ++k) one(qlen, tlen, h0, dir, dir, rev != 0, edge, mm[k], -1, -1, OPT_W);
				if (qlen >= 2) { const int p1 = rnd(qlen), p2 = (p1 + 1 + rnd(qlen - 1)) % qlen; one(qlen, tlen, h0, dir, dir, rev != 0, edge, p1, p2, -1, OPT_W); }
				one(qlen, tlen, h0, dir, dir, rev != 0, edge, -1, -1, rnd(qlen), OPT_W);
				one(qlen, tlen, h0, dir, dir, rev != 0, edge, rnd(qlen), -1, rnd(qlen), OPT_W << 1);
			}
		}
	}
	for (int it = 0; it < iters; ++it) {
		if (it % 64 == 0) new_strand();
		const int qlen = 1 + (rnd(3) == 0 ? rnd(12) : rnd(255)), tlen = rnd(8) == 0 ? qlen - 1 + rnd(2) : qlen + rnd(201);
		const int h0 = rnd(6) == 0 ? 1 + rnd(8) : 19 + rnd(132), shape = rnd(8);
		one(qlen, tlen, h0, rnd(2) ? 1 : -1, rnd(2) ? 1 : -1, rnd(2) == 1, rnd(3), shape < 6 ? rnd(qlen) : -1, shape == 5 ? rnd(qlen) : -1, shape == 7 ? rnd(qlen) : -1, OPT_W << rnd(3));
	}
	return out[0];
}

// tests/recsim/rec_sim.cpp -- TEST PROGRAM, not part of the product.
//
// The functors of arachne_amd/csrc/dev_records.h (what arx_batch_records launches) compiled for the host and run as plain loops over their
// items on random cases, every array allocated at exactly the size the stage driver gives it, so that a read or write past an end shows under
// -fsanitize=address,undefined.  The stream they write is compared byte for byte with the host path on the same case: RecBuf::build
// (bam_records.h) followed by BamSink::encode (bam_sink.h).  Both sides call bam_rules.h, so the program also prints a 64-bit digest of the
// host path's stream for a test to pin.  Usage: rec_sim <seed> <cases> [rev]   (rev: items in descending order) -> "<cases> <digest>"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../arachne_amd/csrc/dev_records.h"
#include "../../arachne_amd/csrc/bam_records.h"
#include "../../arachne_amd/csrc/bam_sink.h"

using namespace arx;
static_assert(sizeof(arx_cand) == sizeof(Cand) && sizeof(arx_aln) == sizeof(Aln) && sizeof(arx_cand_post) == sizeof(CandPost), "C-ABI structs mirror the device structs");

static uint64_t g_x, g_digest = 0xcbf29ce484222325ull; // FNV-1a over the host path's stream of every case
static int rnd(int m) { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return (int)(g_x % (uint64_t)m); }
template <class T> static T *exact(const std::vector<T> &v) { T *p = (T *)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0)); if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); return p; }
template <class F> static void items(int n, bool rev, const F &f) { if (rev) for (int i = n - 1; i >= 0; --i) f(i, 0); else for (int i = 0; i < n; ++i) f(i, 0); }

static bool one_case(int it, bool rev, bool dup)
{
	const int P = 1 + rnd(it % 5 == 0 ? 3 : 40), R = 2 * P;
	// the super-batch
	std::vector<int32_t> lens(R), base_off(R + 1, 0);
	for (int r = 0; r < R; ++r) { const int k = rnd(8); lens[r] = k == 0 ? 0 : k == 1 ? 255 : k == 2 ? 1 + rnd(20) : 18 + rnd(238); base_off[r + 1] = base_off[r] + lens[r]; }
	const int NB = base_off[R];
	std::vector<uint8_t> bases(NB); std::vector<char> quals(NB);
	for (int i = 0; i < NB; ++i) { bases[i] = (uint8_t)(rnd(20) == 0 ? 4 : rnd(4)); quals[i] = (char)(33 + rnd(94)); }
	std::vector<int64_t> name_off(P + 1, 0), rg_off(P + 1, 0);
	std::string names, rgs;
	for (int p = 0; p < P; ++p) {
		const int k = rnd(6), nl = k == 0 ? 1 : k == 1 ? 254 : 1 + rnd(60), rl = rnd(3) == 0 ? 0 : 1 + rnd(24);
		for (int j = 0; j < nl; ++j) names += (char)('!' + rnd(90));
		for (int j = 0; j < rl; ++j) rgs += (char)('A' + rnd(26));
		name_off[p + 1] = (int64_t)names.size(); rg_off[p + 1] = (int64_t)rgs.size();
	}
	std::vector<int64_t> set_off(1, 0), bc_off(1, 0);
	std::string bcs; std::vector<uint8_t> uniq;
	while (set_off.back() < P) {
		const int64_t n = rnd(7) == 0 ? 0 : 1 + rnd(9); // (an empty set now and then: the pair's set is the last one that starts at or before it)
		set_off.push_back(set_off.back() + n > P ? P : set_off.back() + n);
		const int bl = rnd(8) == 0 ? 0 : 4 + rnd(20);
		for (int j = 0; j < bl; ++j) bcs += (char)(rnd(5) == 0 ? '-' : 'A' + rnd(4));
		bc_off.push_back((int64_t)bcs.size()); uniq.push_back((uint8_t)(rnd(4) != 0));
	}
	const int NS = (int)uniq.size();
	names += '\0'; rgs += '\0'; bcs += '\0'; // (the host path's arrays may be followed by anything; the device's copies below end exactly)
	arx_super_batch sb;
	memset(&sb, 0, sizeof sb);
	sb.n_sets = NS; sb.n_pairs = P; sb.set_pair_off = set_off.data(); sb.unique = uniq.data(); sb.bases = bases.data(); sb.quals = quals.data(); sb.lens = lens.data();
	sb.name_off = name_off.data(); sb.names = names.data(); sb.rg_off = rg_off.data(); sb.rgs = rgs.data(); sb.barcode_off = bc_off.data(); sb.barcodes = bcs.data();
	// candidates, alignments, CIGARs
	std::vector<int32_t> cand_off(R + 1, 0);
	std::vector<Cand> cands; std::vector<Aln> alns; std::vector<uint32_t> cig; std::vector<CandPost> post;
	for (int r = 0; r < R; ++r) {
		const int n = 1 + rnd(4), act = rnd(n), act2 = rnd(3) == 0 ? rnd(n) : act; // sometimes two active ones: the last counts
		for (int i = 0; i < n; ++i) {
			Cand c = Cand();
			const bool ph = n == 1 && rnd(4) == 0;
			c.read = r; c.rid = ph ? -1 : rnd(3); c.reversed = rnd(2); c.score = rnd(3) == 0 ? 19 + rnd(20) : 30 + rnd(230); c.is_proper = rnd(2); c.mapq = rnd(300) - 20;
			c.active = i == act || i == act2; c.active_molecule = rnd(2);
			c.pos = ph ? -1 : (rnd(5) == 0 ? (int64_t)rnd(1 << 30) : (int64_t)rnd(200000)); c.aend = c.pos + 1 + rnd(400);
			c.reg = -1;
			if (!ph) {
				Aln a = Aln();
				a.n_cigar = rnd(6) == 0 ? 0 : 1 + rnd(7); a.cigar_off = (int32_t)cig.size();
				for (int k = 0; k < a.n_cigar; ++k) cig.push_back((uint32_t)(1 + rnd(rnd(9) == 0 ? 40000 : 120)) << 4 | (uint32_t)(rnd(30) == 0 ? 5 + rnd(4) : rnd(5)));
				c.reg = (int32_t)alns.size(); alns.push_back(a);
			}
			CandPost cp = CandPost(); cp.duplicate = rnd(3) == 0;
			cands.push_back(c); post.push_back(cp);
		}
		cand_off[r + 1] = (int32_t)cands.size();
	}
	// ---- the host path
	RecBuf rb; arx_bam_batch view; std::string err;
	if (!rb.build(sb, cand_off.data(), (const arx_cand *)cands.data(), (const arx_aln *)alns.data(), cig.data(), dup ? (const arx_cand_post *)post.data() : nullptr, 2, &view, err)) { fprintf(stderr, "host build: %s\n", err.c_str()); return false; }
	std::vector<uint8_t> want; std::vector<size_t> woff(R + 1, 0);
	for (int r = 0; r < R; ++r) woff[r + 1] = woff[r] + BamSink::record_size(view, r);
	want.resize(woff[R]);
	for (int r = 0; r < R; ++r) BamSink::encode(view, r, want.data() + woff[r]);
	for (uint8_t b : want) g_digest = (g_digest ^ b) * 0x100000001b3ull;
	// ---- the device functors on arrays of exactly the driver's sizes
	std::vector<uint8_t> bx(NS);
	for (int s = 0; s < NS; ++s) bx[s] = bam_set_bx(uniq[s], bcs.data() + bc_off[s], bc_off[s + 1] - bc_off[s]);
	std::vector<uint8_t> q8(quals.begin(), quals.end()), nm8(names.begin(), names.end() - 1), rg8(rgs.begin(), rgs.end() - 1), bc8(bcs.begin(), bcs.end() - 1);
	RecInputs in;
	uint8_t *d_q = exact(q8), *d_nm = exact(nm8), *d_rg = exact(rg8), *d_bc = exact(bc8), *d_bx = exact(bx), *d_bases = exact(bases);
	int64_t *d_no = exact(name_off), *d_ro = exact(rg_off), *d_bo = exact(bc_off), *d_so = exact(set_off);
	in.quals = d_q; in.names = d_nm; in.name_off = d_no; in.rgs = d_rg; in.rg_off = d_ro; in.barcodes = d_bc; in.barcode_off = d_bo; in.set_pair_off = d_so; in.set_bx = d_bx; in.n_sets = NS;
	Cand *d_cands = exact(cands); Aln *d_alns = exact(alns); uint32_t *d_cig = exact(cig); CandPost *d_post = exact(post);
	int32_t *d_co = exact(cand_off), *d_lens = exact(lens), *d_boff = exact(base_off);
	RecMeta *meta = (RecMeta *)malloc(sizeof(RecMeta) * (size_t)R);
	int32_t *size = (int32_t *)malloc(4 * (size_t)R), *rec_off = (int32_t *)malloc(4 * ((size_t)R + 1));
	uint32_t e = 0;
	items(R, rev, KBamRecSize{d_cands, d_co, d_alns, d_cig, dup ? d_post : nullptr, d_lens, d_boff, in, meta, size, &e});
	int64_t total = 0;
	for (int r = 0; r < R; ++r) { rec_off[r] = (int32_t)total; total += size[r]; }
	rec_off[R] = (int32_t)total;
	bool ok = e == 0 && (size_t)total == want.size();
	if (!ok) fprintf(stderr, "case %d: error word %u, %lld bytes against %zu\n", it, e, (long long)total, want.size());
	const int n_words = (int)((total + 15) / 16), n_tiles = (int)((total + REC_TILE - 1) / REC_TILE);
	int32_t *tile_first = (int32_t *)malloc(4 * (size_t)(n_tiles ? n_tiles : 1));
	RecWord16 *out = (RecWord16 *)aligned_alloc(16, 16 * (size_t)(n_words ? n_words : 1));
	memset(out, 0xAB, 16 * (size_t)(n_words ? n_words : 1));
	if (ok) {
		items(n_tiles, rev, KBamRecTile{rec_off, R, tile_first});
		items(n_words, rev, KBamRecFill{RecSources{d_cig, d_bases, in}, meta, rec_off, tile_first, R, total, out});
		const uint8_t *got = (const uint8_t *)out;
		for (int64_t i = 0; i < 16 * (int64_t)n_words && ok; ++i) {
			const uint8_t w = i < total ? want[(size_t)i] : 0; // bytes of the last word past the stream are zero
			if (got[i] != w) { fprintf(stderr, "case %d: byte %lld of %lld is %u, the host path has %u\n", it, (long long)i, (long long)total, got[i], w); ok = false; }
		}
		for (int r = 0; r <= R && ok; ++r) if ((size_t)rec_off[r] != woff[r]) { fprintf(stderr, "case %d: record %d starts at %d against %zu\n", it, r, rec_off[r], woff[r]); ok = false; }
	}
	void *all[] = {d_q, d_nm, d_rg, d_bc, d_bx, d_bases, d_no, d_ro, d_bo, d_so, d_cands, d_alns, d_cig, d_post, d_co, d_lens, d_boff, meta, size, rec_off, tile_first, out};
	for (void *p : all) free(p);
	return ok;
}

int main(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: rec_sim <seed> <cases> [rev]\n"); return 2; }
	g_x = 0x9E3779B97F4A7C15ull * (uint64_t)(atoi(argv[1]) + 1);
	const int n = atoi(argv[2]);
	const bool rev = argc > 3 && !strcmp(argv[3], "rev");
	for (int it = 0; it < n; ++it) if (!one_case(it, rev, (it & 1) != 0)) return 1;
	printf("%d %016llx\n", n, (unsigned long long)g_digest);
	return 0;
}

// tests/recsim/rec_full_sim.cpp -- TEST PROGRAM, not part of the product.
//
// The functors of arachne_amd/csrc/dev_records_full.h (what arx_batch_records_full launches) compiled for the host and run as plain loops over
// their items on random cases, every array allocated at exactly the size the functors may touch, so that a read or write past an end shows
// under -fsanitize=address,undefined.  Both streams, bucket[] and both offset tables are compared with the host path on the same case:
// RecBuf::build in its full mode (bam_records.h) followed by BamSink::encode (bam_sink.h), and the stable order of that by bucket.  The cases
// hold what the path cannot reach at test size: primaries the score rule unmaps that have a split, splits it unmaps, hard clips that eat the
// whole read, mismatch lists of 0, 1 and 300+ entries with values of 1 to 10 digits and negative ones, CIGARs of 1 to 40+ words, contig names of
// 1 and 60+ bytes, empty read groups and barcodes, sets without BX, dm_n = 0, 1 to 300+ buckets with empty ones, all records in one bucket.
// Both sides call bam_rules.h, so the program also prints a 64-bit digest of the HOST path's stream and buckets for a test to pin.
//   rec_full_sim <seed> <cases> [rev]   (rev: items in descending order)   -> "<cases> <digest>"
//   rec_full_sim text                   the two decimal formatters against snprintf    -> "<%.6f cases> <ties> <%d cases>"
// -DREC_FULL_SIM_HOST_ONLY leaves the device side out (no dev_records_full.h): the form that compiles against the tree as it was before the
// rules moved into bam_rules.h, which is how the pinned digest was made.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#ifndef REC_FULL_SIM_HOST_ONLY
#include "../../arachne_amd/csrc/dev_records_full.h"
#else
#include "../../arachne_amd/csrc/dev_post.h"
#endif
#include "../../arachne_amd/csrc/bam_records.h"
#include "../../arachne_amd/csrc/bam_sink.h"

using namespace arx;
static_assert(sizeof(arx_cand) == sizeof(Cand) && sizeof(arx_aln) == sizeof(Aln) && sizeof(arx_cand_post) == sizeof(CandPost) && sizeof(arx_split) == sizeof(SplitRec) &&
              sizeof(arx_read_tags) == sizeof(ReadTags), "C-ABI structs mirror the device structs");

static uint64_t g_x, g_digest = 0xcbf29ce484222325ull; // FNV-1a over the host path's stream and buckets of every case
static int rnd(int m) { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return (int)(g_x % (uint64_t)m); }
static void digest(const void *p, size_t n) { for (size_t i = 0; i < n; ++i) g_digest = (g_digest ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull; }
template <class T> static T *exact(const std::vector<T> &v) { T *p = (T *)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0)); if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); return p; }
template <class T> static T *room(size_t n) { return (T *)malloc(n * sizeof(T) + (n ? 0 : 1)); }
template <class F> static void items(int n, bool rev, const F &f) { if (rev) for (int i = n - 1; i >= 0; --i) f(i, 0); else for (int i = 0; i < n; ++i) f(i, 0); }
static int32_t mm_value() // 1 to 10 digits, now and then negative
{
	static const int64_t top[10] = {10, 100, 1000, 10000, 100000, 1000000, 10000000, 100000000, 1000000000, 2147483647};
	const int d = rnd(10);
	const int32_t v = (int32_t)(((uint64_t)rnd(1 << 30) * 4 + rnd(4)) % (uint64_t)top[d]);
	return rnd(6) == 0 ? -v - (rnd(50) == 0 ? 1 : 0) : v;
}

// what the cases must have held by the end of a run of 100 or more: counted from the host path's inputs and results
enum { COV_PRIMARY_UNMAPPED_SPLIT, COV_SPLIT_UNMAPPED, COV_CLIPPED_AWAY, COV_MM_0, COV_MM_1, COV_MM_300, COV_SA_CIGAR_40, COV_SA_CIGAR_1, COV_CONTIG_1, COV_CONTIG_60, COV_NO_RG, COV_NO_BARCODE,
       COV_NO_BX, COV_DM_N_0, COV_DM, COV_FILES_300, COV_FILES_2, COV_ONE_BUCKET, COV_EMPTY_BUCKET, COV_N };
static long g_cov[COV_N + 1]; // (the last: everything else)
static const char *const g_cov_name[COV_N] = {"primary unmapped with a split", "split unmapped", "hard clips >= read", "empty list", "list of 1", "list of 300+", "SA CIGAR of 40+", "SA CIGAR of 1", "contig name of 1",
	"contig name of 60+", "empty read group", "empty barcode", "set without BX", "dm_n = 0", "DM written", "300+ buckets", "2 buckets", "all records in one bucket", "an empty bucket"};

static bool one_case(int it, bool rev)
{
	const int kind = it % 7; // 3: everything in one bucket; 4: 300+ buckets; 5: a single pair
	const int P = kind == 5 ? 1 : 1 + rnd(30), R = 2 * P;
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
		const int64_t n = rnd(7) == 0 ? 0 : 1 + rnd(9);
		set_off.push_back(set_off.back() + n > P ? P : set_off.back() + n);
		const int bl = rnd(8) == 0 ? 0 : 4 + rnd(20);
		for (int j = 0; j < bl; ++j) bcs += (char)(rnd(5) == 0 ? '-' : 'A' + rnd(4));
		bc_off.push_back((int64_t)bcs.size()); uniq.push_back((uint8_t)(rnd(4) != 0));
	}
	const int NS = (int)uniq.size();
	names += '\0'; rgs += '\0'; bcs += '\0';
	arx_super_batch sb;
	memset(&sb, 0, sizeof sb);
	sb.n_sets = NS; sb.n_pairs = P; sb.set_pair_off = set_off.data(); sb.unique = uniq.data(); sb.bases = bases.data(); sb.quals = quals.data(); sb.lens = lens.data();
	sb.name_off = name_off.data(); sb.names = names.data(); sb.rg_off = rg_off.data(); sb.rgs = rgs.data(); sb.barcode_off = bc_off.data(); sb.barcodes = bcs.data();
	// contigs and the bucket table: contig i owns n_chunk files, the unmapped file comes last
	const int NCtg = kind == 3 ? 1 : 1 + rnd(5);
	const int64_t max_pos = kind == 4 ? 40000 : 200000, chunk = kind == 3 ? 1000000000 : kind == 4 ? 100 : 1 + rnd(3) * 30000 + rnd(70000);
	std::vector<std::string> ctg(NCtg);
	std::vector<const char *> ctg_ptr(NCtg);
	std::vector<int32_t> contig_file(NCtg), ctg_off(1, 0);
	std::string ctg_all;
	int32_t n_files = 0;
	for (int i = 0; i < NCtg; ++i) {
		const int nl = rnd(3) == 0 ? 1 : rnd(2) ? 60 + rnd(30) : 2 + rnd(12);
		for (int j = 0; j < nl; ++j) ctg[i] += (char)('a' + rnd(26));
		ctg_ptr[i] = ctg[i].c_str(); ctg_all += ctg[i]; ctg_off.push_back((int32_t)ctg_all.size());
		contig_file[i] = n_files; n_files += (int32_t)(max_pos / chunk) + 1;
	}
	const int32_t unmapped_file = n_files++;
	// candidates, alignments, CIGARs, the post and tags phases' records
	std::vector<int32_t> cand_off(R + 1, 0), mm_ref, mm_read;
	std::vector<Cand> cands; std::vector<Aln> alns; std::vector<uint32_t> cig; std::vector<CandPost> post;
	std::vector<SplitRec> split(R); std::vector<ReadTags> tags(R);
	for (int r = 0; r < R; ++r) {
		const int n = 1 + rnd(4), act = rnd(n), act2 = rnd(3) == 0 ? rnd(n) : act;
		for (int i = 0; i < n; ++i) {
			Cand c = Cand();
			const bool ph = kind != 3 && n == 1 && rnd(4) == 0;
			c.read = r; c.rid = ph ? -1 : rnd(NCtg); c.reversed = rnd(2); c.score = ph ? 0 : rnd(3) == 0 ? 19 + rnd(20) : 30 + rnd(230); c.is_proper = ph ? 0 : kind == 3 ? 1 : rnd(2); c.mapq = rnd(300) - 20;
			c.active = i == act || i == act2; c.active_molecule = rnd(2);
			c.pos = ph ? -1 : (int64_t)rnd((int)max_pos); c.aend = c.pos + 1 + rnd(400);
			c.reg = -1;
			if (!ph) {
				Aln a = Aln();
				a.n_cigar = rnd(12) == 0 ? 0 : rnd(10) == 0 ? 40 + rnd(30) : 1 + rnd(7); a.cigar_off = (int32_t)cig.size();
				for (int k = 0; k < a.n_cigar; ++k) {
					uint32_t op = (uint32_t)(rnd(30) == 0 ? 5 + rnd(4) : rnd(5));
					if ((k == 0 || k == a.n_cigar - 1) && rnd(2)) op = 3; // soft clips at the ends: the split record's hard clips
					cig.push_back((uint32_t)(1 + rnd(rnd(9) == 0 ? 40000 : rnd(4) == 0 ? 300 : 60)) << 4 | op);
				}
				c.reg = (int32_t)alns.size(); alns.push_back(a);
			}
			CandPost cp = CandPost();
			cp.duplicate = rnd(3) == 0; cp.qb = rnd(50); cp.qe = 50 + rnd(200); cp.matches = rnd(250);
			const int k = rnd(8);
			cp.n_mm = ph || k < 2 ? 0 : k == 2 ? 1 : rnd(40) == 0 ? 300 + rnd(80) : 2 + rnd(12);
			cp.mm_off = (int32_t)mm_ref.size();
			for (int j = 0; j < cp.n_mm; ++j) { mm_ref.push_back(mm_value()); mm_read.push_back(rnd(3) ? rnd(256) : mm_value()); }
			cands.push_back(c); post.push_back(cp);
		}
		cand_off[r + 1] = (int32_t)cands.size();
	}
	const int NC = (int)cands.size();
	for (int r = 0; r < R; ++r) {
		SplitRec s = SplitRec();
		s.split = -1;
		if (rnd(3) == 0) { const int i = cand_off[r] + rnd(cand_off[r + 1] - cand_off[r]); if (cands[i].reg >= 0) s.split = i; }
		s.mapq = rnd(300) - 20; s.is_proper = kind == 3 ? 1 : rnd(2); s.n_split_cand = rnd(5); s.order_pinned = 1;
		s.second_best2 = rnd(2) ? rnd(600) - 300 : -1 - 2 * rnd(100); s.score2 = rnd(2) ? rnd(600) - 300 : -1 - 2 * rnd(100);
		split[r] = s;
		ReadTags t = ReadTags();
		t.active = cand_off[r]; t.second_best = rnd(3) == 0 ? -1 : rnd(NC);
		t.xs = rnd(4) == 0 ? -rnd(1 << 30) : rnd(300); t.as = rnd(4) == 0 ? INT_MIN + rnd(3) : rnd(300); t.xm = rnd(2); t.xt = rnd(2);
		t.dm_n = rnd(4) == 0 ? 0 : rnd(3) == 0 ? 1 + rnd(60000) : 1 + rnd(40);
		t.dm_sum = rnd(5) == 0 ? (int32_t)(((uint32_t)rnd(1 << 30) << 1 | (uint32_t)rnd(2)) & 0x7fffffffu) : rnd(4 * t.dm_n + 1);
		tags[r] = t;
	}
	// ---- the host path
	arx_recbuf_full full;
	memset(&full, 0, sizeof full);
	full.split = (const arx_split *)split.data(); full.mm_ref = mm_ref.data(); full.mm_read = mm_read.data(); full.tags = (const arx_read_tags *)tags.data();
	full.n_contigs = NCtg; full.contig_names = ctg_ptr.data(); full.contig_file = contig_file.data(); full.chunk = chunk; full.unmapped_file = unmapped_file;
	RecBuf rb; arx_bam_batch view; std::string err;
	if (!rb.build(sb, cand_off.data(), (const arx_cand *)cands.data(), (const arx_aln *)alns.data(), cig.data(), (const arx_cand_post *)post.data(), 2, &view, err, &full)) { fprintf(stderr, "host build: %s\n", err.c_str()); return false; }
	const int NRec = (int)view.n_records;
	std::vector<uint8_t> want; std::vector<size_t> woff(NRec + 1, 0);
	for (int q = 0; q < NRec; ++q) woff[q + 1] = woff[q] + BamSink::record_size(view, q);
	want.resize(woff[NRec]);
	for (int q = 0; q < NRec; ++q) BamSink::encode(view, q, want.data() + woff[q]);
	digest(want.data(), want.size()); digest(rb.bucket.data(), 4 * rb.bucket.size());
#ifndef REC_FULL_SIM_HOST_ONLY
	for (int r = 0; r < R; ++r) { // coverage
		const BamReadState st = bam_read_state((const arx_cand *)cands.data(), (const arx_aln *)alns.data(), cig.data(), rb.act[r], rb.act[r ^ 1], split[r], r);
		const int p = r >> 1; int s = 0;
		while (!(set_off[s] <= p && p < set_off[s + 1])) ++s;
		const bool bx = bam_set_bx(uniq[s], bcs.data() + bc_off[s], bc_off[s + 1] - bc_off[s]);
		auto list = [&](int c) { if (c < 0) return; const int n = post[c].n_mm; ++g_cov[n == 0 ? COV_MM_0 : n == 1 ? COV_MM_1 : n >= 300 ? COV_MM_300 : COV_N]; };
		auto sa = [&](int c) { const int n = alns[cands[c].reg].n_cigar; if (n >= 40) ++g_cov[COV_SA_CIGAR_40]; if (n == 1) ++g_cov[COV_SA_CIGAR_1]; const size_t l = ctg[cands[c].rid].size(); if (l == 1) ++g_cov[COV_CONTIG_1]; if (l >= 60) ++g_cov[COV_CONTIG_60]; };
		list(tags[r].second_best); list(st.a);
		if (rg_off[p + 1] == rg_off[p]) ++g_cov[COV_NO_RG];
		if (bc_off[s + 1] == bc_off[s]) ++g_cov[COV_NO_BARCODE];
		if (!bx) ++g_cov[COV_NO_BX];
		if (bx && cands[st.a].active_molecule) ++g_cov[tags[r].dm_n == 0 ? COV_DM_N_0 : COV_DM];
		if (st.s >= 0) {
			list(st.s); sa(st.s);
			if (st.cpos == -1) ++g_cov[COV_PRIMARY_UNMAPPED_SPLIT]; else sa(st.a);
			if (st.spos == -1) ++g_cov[COV_SPLIT_UNMAPPED];
			if (lens[r] > 0 && st.hc0 + st.hc1 >= lens[r]) ++g_cov[COV_CLIPPED_AWAY];
		}
	}
	{
		std::vector<int> per(n_files, 0);
		for (int32_t b : rb.bucket) ++per[b];
		if (n_files >= 300) ++g_cov[COV_FILES_300];
		if (n_files == 2) ++g_cov[COV_FILES_2];
		if (*std::max_element(per.begin(), per.end()) == NRec) ++g_cov[COV_ONE_BUCKET];
		if (*std::min_element(per.begin(), per.end()) == 0) ++g_cov[COV_EMPTY_BUCKET];
	}
#endif
	// the stable order by bucket and the grouped stream
	std::vector<int> ord(NRec);
	for (int q = 0; q < NRec; ++q) ord[q] = q;
	std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return rb.bucket[a] < rb.bucket[b]; });
	std::vector<uint8_t> want_g; std::vector<int64_t> want_boff(n_files + 1, 0), want_roff(n_files + 1, 0);
	for (int j = 0, f = 0; j <= NRec; ++j) {
		const int bk = j < NRec ? rb.bucket[ord[j]] : n_files;
		for (; f <= bk && f <= n_files; ++f) { want_roff[f] = j; want_boff[f] = (int64_t)want_g.size(); }
		if (j < NRec) want_g.insert(want_g.end(), want.begin() + woff[ord[j]], want.begin() + woff[ord[j] + 1]);
	}
#ifdef REC_FULL_SIM_HOST_ONLY
	(void)rev;
	return true;
#else
	// ---- the device functors on arrays of exactly the sizes they may touch
	std::vector<uint8_t> bx(NS);
	for (int s = 0; s < NS; ++s) bx[s] = bam_set_bx(uniq[s], bcs.data() + bc_off[s], bc_off[s + 1] - bc_off[s]);
	std::vector<uint8_t> q8(quals.begin(), quals.end()), nm8(names.begin(), names.end() - 1), rg8(rgs.begin(), rgs.end() - 1), bc8(bcs.begin(), bcs.end() - 1), ctg8(ctg_all.begin(), ctg_all.end());
	RecInputs in;
	uint8_t *d_q = exact(q8), *d_nm = exact(nm8), *d_rg = exact(rg8), *d_bc = exact(bc8), *d_bx = exact(bx), *d_bases = exact(bases), *d_ctg = exact(ctg8);
	int64_t *d_no = exact(name_off), *d_ro = exact(rg_off), *d_bo = exact(bc_off), *d_so = exact(set_off);
	in.quals = d_q; in.names = d_nm; in.name_off = d_no; in.rgs = d_rg; in.rg_off = d_ro; in.barcodes = d_bc; in.barcode_off = d_bo; in.set_pair_off = d_so; in.set_bx = d_bx; in.n_sets = NS;
	Cand *d_cands = exact(cands); Aln *d_alns = exact(alns); uint32_t *d_cig = exact(cig); CandPost *d_post = exact(post);
	SplitRec *d_split = exact(split); ReadTags *d_tags = exact(tags);
	int32_t *d_co = exact(cand_off), *d_lens = exact(lens), *d_boff = exact(base_off), *d_mr = exact(mm_ref), *d_mq = exact(mm_read), *d_cf = exact(contig_file), *d_cno = exact(ctg_off);
	const int NM = (int)mm_ref.size();
	int32_t *mm_len = room<int32_t>(NM), *mm_txt = room<int32_t>(NM + 1);
	items(NM, rev, KRecMmLen{d_mr, d_mq, mm_len});
	{ int64_t t = 0; for (int e = 0; e < NM; ++e) { mm_txt[e] = (int32_t)t; t += mm_len[e]; } mm_txt[NM] = (int32_t)t; }
	RecFullInputs F;
	F.post = d_post; F.split = d_split; F.tags = d_tags; F.mm_ref = d_mr; F.mm_read = d_mq; F.mm_txt_off = mm_txt; F.contig_names = d_ctg; F.contig_name_off = d_cno;
	F.contig_file = d_cf; F.n_contigs = NCtg; F.unmapped_file = unmapped_file; F.chunk = chunk;
	int32_t *n_rec = room<int32_t>(R), *rbase = room<int32_t>(R + 1);
	uint32_t e = 0;
	items(R, rev, KRecFullCount{d_cands, d_co, d_split, n_rec, &e});
	int got_rec = 0;
	for (int r = 0; r < R; ++r) { rbase[r] = got_rec; got_rec += n_rec[r]; }
	rbase[R] = got_rec;
	bool ok = e == 0 && got_rec == NRec;
	if (!ok) fprintf(stderr, "case %d: error word %u, %d records against %d\n", it, e, got_rec, NRec);
	RecFullMeta *meta = room<RecFullMeta>(NRec);
	int32_t *size = room<int32_t>(NRec), *bucket = room<int32_t>(NRec), *rec_off = room<int32_t>(NRec + 1);
	int32_t *order = room<int32_t>(NRec), *gsize = room<int32_t>(NRec), *g_off = room<int32_t>(NRec + 1);
	int64_t *b_rec = room<int64_t>(n_files + 1), *b_byte = room<int64_t>(n_files + 1);
	int64_t total = 0;
	if (ok) {
		items(R, rev, KRecFullMeta{d_cands, d_co, d_alns, d_cig, d_lens, d_boff, in, F, rbase, meta, size, bucket, &e});
		for (int q = 0; q < NRec; ++q) { rec_off[q] = (int32_t)total; total += size[q]; }
		rec_off[NRec] = (int32_t)total;
		ok = e == 0 && (size_t)total == want.size();
		if (!ok) fprintf(stderr, "case %d: error word %u, %lld bytes against %zu\n", it, e, (long long)total, want.size());
		for (int q = 0; q <= NRec && ok; ++q) if ((size_t)rec_off[q] != woff[q]) { fprintf(stderr, "case %d: record %d starts at %d against %zu\n", it, q, rec_off[q], woff[q]); ok = false; }
		for (int q = 0; q < NRec && ok; ++q) if (bucket[q] != rb.bucket[q]) { fprintf(stderr, "case %d: record %d in bucket %d against %d\n", it, q, bucket[q], rb.bucket[q]); ok = false; }
	}
	const int n_words = (int)((total + 15) / 16), n_tiles = (int)((total + REC_TILE - 1) / REC_TILE);
	int32_t *tile_first = room<int32_t>(n_tiles), *g_tile = room<int32_t>(n_tiles);
	RecWord16 *out = (RecWord16 *)aligned_alloc(16, 16 * (size_t)(n_words ? n_words : 1)), *out_g = (RecWord16 *)aligned_alloc(16, 16 * (size_t)(n_words ? n_words : 1));
	memset(out, 0xAB, 16 * (size_t)(n_words ? n_words : 1)); memset(out_g, 0xAB, 16 * (size_t)(n_words ? n_words : 1));
	const int NBk = (NRec + REC_GROUP_BLOCK - 1) / REC_GROUP_BLOCK;
	const size_t n_tab = (size_t)n_files * NBk;
	int32_t *cnt = room<int32_t>(n_tab), *base = room<int32_t>(n_tab + 1);
	auto same = [&](const char *what, const RecWord16 *o, const std::vector<uint8_t> &w) {
		const uint8_t *got = (const uint8_t *)o;
		for (int64_t i = 0; i < 16 * (int64_t)n_words; ++i) {
			const uint8_t x = i < total ? w[(size_t)i] : 0; // bytes of the last word past the stream are zero
			if (got[i] != x) { fprintf(stderr, "case %d: byte %lld of %lld of the %s stream is %u, the host path has %u\n", it, (long long)i, (long long)total, what, got[i], x); return false; }
		}
		return true;
	};
	if (ok) {
		const RecFullSources S{d_cig, d_bases, in, F};
		items(n_tiles, rev, KBamRecTile{rec_off, NRec, tile_first});
		items(n_words, rev, KRecFullFill{S, meta, nullptr, rec_off, tile_first, NRec, total, out});
		ok = same("record", out, want);
		memset(cnt, 0, 4 * n_tab);
		items(NBk, rev, KRecGroupCount{bucket, NRec, NBk, cnt});
		{ int64_t t = 0; for (size_t i = 0; i < n_tab; ++i) { base[i] = (int32_t)t; t += cnt[i]; } base[n_tab] = (int32_t)t; }
		memset(cnt, 0, 4 * n_tab);
		items(NBk, rev, KRecGroupRank{bucket, base, NRec, NBk, cnt, order});
		items(NRec, rev, KRecGroupSize{size, order, gsize});
		{ int64_t t = 0; for (int j = 0; j < NRec; ++j) { g_off[j] = (int32_t)t; t += gsize[j]; } g_off[NRec] = (int32_t)t; }
		items(n_files + 1, rev, KRecGroupOff{base, g_off, n_files, NBk, NRec, b_rec, b_byte});
		items(n_tiles, rev, KBamRecTile{g_off, NRec, g_tile});
		items(n_words, rev, KRecFullFill{S, meta, order, g_off, g_tile, NRec, total, out_g});
		for (int j = 0; j < NRec && ok; ++j) if (order[j] != ord[j]) { fprintf(stderr, "case %d: grouped record %d is %d against %d\n", it, j, order[j], ord[j]); ok = false; }
		for (int f = 0; f <= n_files && ok; ++f) if (b_rec[f] != want_roff[f] || b_byte[f] != want_boff[f]) { fprintf(stderr, "case %d: bucket %d starts at record %lld byte %lld against %lld, %lld\n", it, f, (long long)b_rec[f], (long long)b_byte[f], (long long)want_roff[f], (long long)want_boff[f]); ok = false; }
		ok = ok && same("grouped", out_g, want_g);
	}
	void *all[] = {d_q, d_nm, d_rg, d_bc, d_bx, d_bases, d_ctg, d_no, d_ro, d_bo, d_so, d_cands, d_alns, d_cig, d_post, d_split, d_tags, d_co, d_lens, d_boff, d_mr, d_mq, d_cf, d_cno, mm_len, mm_txt,
	               n_rec, rbase, meta, size, bucket, rec_off, order, gsize, g_off, b_rec, b_byte, tile_first, g_tile, out, out_g, cnt, base};
	for (void *p : all) free(p);
	return ok;
#endif
}

#ifndef REC_FULL_SIM_HOST_ONLY
static std::string dev_int(int32_t v) { std::string s; for (int i = 0, l = int_len(v); i < l; ++i) s += (char)int_char(v, i); return s; }
static std::string dev_dm(int32_t s, int32_t n) { const uint64_t t = dm_scaled_signed(s, n); std::string o; for (int i = 0, l = dm_len(s, t); i < l; ++i) o += (char)dm_char(s < 0, t, i); return o; }
static bool dm_same(int32_t s, int32_t n)
{
	char b[64];
	snprintf(b, sizeof b, "%.6f", (double)s / (double)n);
	if (dev_dm(s, n) == b) return true;
	fprintf(stderr, "%%.6f of %d / %d: %s against snprintf's %s\n", s, n, dev_dm(s, n).c_str(), b);
	return false;
}
static int text_mode()
{
	long n_dm = 0, n_tie = 0, n_int = 0;
	for (int n = 1; n <= 512; ++n) for (int s = 0; s <= 4 * n; ++s, ++n_dm) if (!dm_same(s, n)) return 1;
	// every tie: 2 s 10^6 / n an odd integer, which needs 128 | n
	for (int n = 128; n <= 32768; n += 128) for (int s = 0; s <= 4 * n; ++s) {
		const int64_t a = 2000000ll * s;
		if (a % n || !((a / n) & 1)) continue;
		++n_tie;
		if (!dm_same(s, n)) return 1;
	}
	for (int k = 0; k < 200000; ++k, ++n_dm) { const int n = 1 + rnd(60000); const int32_t s = (int32_t)(((uint32_t)rnd(1 << 30) << 1 | (uint32_t)rnd(2)) & 0x7fffffffu); if (!dm_same(s, n) || !dm_same(-s, n)) return 1; }
	std::vector<int32_t> v = {0, INT_MAX, INT_MIN, INT_MIN + 1};
	for (int64_t p = 1; p <= 1000000000; p *= 10) for (int64_t d = -1; d <= 1; ++d) { v.push_back((int32_t)(p + d)); v.push_back((int32_t)-(p + d)); }
	for (int k = 0; k < 100000; ++k) v.push_back(mm_value());
	for (int32_t x : v) {
		char b[32];
		snprintf(b, sizeof b, "%d", x);
		++n_int;
		if (dev_int(x) != b) { fprintf(stderr, "%%d of %d: %s\n", x, dev_int(x).c_str()); return 1; }
		snprintf(b, sizeof b, "%lld", (long long)x * 4099);
		std::string s64; for (int i = 0, l = int64_len((int64_t)x * 4099); i < l; ++i) s64 += (char)int64_char((int64_t)x * 4099, i);
		if (s64 != b) { fprintf(stderr, "%%lld of %lld: %s\n", (long long)x * 4099, s64.c_str()); return 1; }
	}
	printf("%ld %ld %ld\n", n_dm, n_tie, n_int);
	return 0;
}
#endif

int main(int argc, char **argv)
{
	g_x = 0x9E3779B97F4A7C15ull;
#ifndef REC_FULL_SIM_HOST_ONLY
	if (argc == 2 && !strcmp(argv[1], "text")) return text_mode();
#endif
	if (argc < 3) { fprintf(stderr, "usage: rec_full_sim <seed> <cases> [rev] | rec_full_sim text\n"); return 2; }
	g_x = 0x9E3779B97F4A7C15ull * (uint64_t)(atoi(argv[1]) + 1);
	const int n = atoi(argv[2]);
	const bool rev = argc > 3 && !strcmp(argv[3], "rev");
	for (int it = 0; it < n; ++it) if (!one_case(it, rev)) return 1;
#ifndef REC_FULL_SIM_HOST_ONLY
	if (n >= 100) for (int k = 0; k < COV_N; ++k) if (!g_cov[k]) { fprintf(stderr, "the cases held no %s\n", g_cov_name[k]); return 1; }
#endif
	printf("%d %016llx\n", n, (unsigned long long)g_digest);
	return 0;
}

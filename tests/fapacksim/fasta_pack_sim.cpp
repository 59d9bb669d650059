// tests/fapacksim/fasta_pack_sim.cpp -- TEST PROGRAM, not part of the product: arachne_amd/csrc/dev_fapack.h compiled for the host, the items of a
// launch run one after the other in a loop.  tests/test_fasta_pack_sim.py builds it with -fsanitize=address,undefined and runs it as a plain process.
//
//   fasta_pack_sim MANIFEST OUTDIR    MANIFEST: one case per line, "name fasta_path status claim,claim,..." (status: what the restatement of
//                                     tests/fapackcases.py makes of the text -- 0 packed, 1 a base before the first '>', 2 no base; "-": no
//                                     claim).  Beside fasta_path lie the restatement's files, fasta_path.want.pac / .ann / .amb (status 0).
// Every case runs at window sizes 64, 256 and 4096, the items of every launch in ascending and in descending order: six runs, every buffer an
// allocation of exactly the bytes the orchestration asks its driver for.  The six are held to one another (everything they report), to the
// restatement's status and files, and to build_index itself (index_build.h, with a suffix sorter that does nothing) on the same file.
// Prints per case "case name status l_pac contigs holes ambiguous cnt0 cnt1 cnt2 cnt3", then "contig begin end offset length holes" per contig
// and "hole offset length byte" per hole; OUTDIR/name.pac / .ann / .amb are the files of the first run.
// Exit status 3: two runs disagree; 4: a case did not meet a condition its line claims; 5: the runs differ from the restatement; 6: from
// build_index.  Claims:
//   windows   more than one window at 64 bytes            codes    codes were carried from one window to the next at 64 bytes
//   header    a window's end cut a header at 64 bytes     skew     (the program's own check) the fourth run's first .pac byte is changed
//                                                                  before the runs are compared: exit status 3 is expected
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sstream>
#include <string>
#include <vector>
#include "../../arachne_amd/csrc/dev_fapack.h"
#include "../../arachne_amd/csrc/index_build.h"

using namespace arx;

static void *exact(int64_t bytes) // an allocation of exactly `bytes`, 16-byte aligned: an access past it is the sanitizer's to find
{
	void *p = nullptr;
	if (posix_memalign(&p, 16, (size_t)(bytes ? bytes : 1))) { fprintf(stderr, "out of memory\n"); exit(2); }
	if (bytes) memset(p, 0xA5, (size_t)bytes);
	return p;
}

struct SimDrv {
	bool rev = false;
	void *work_[FA_N_WORK] = {nullptr};
	void *keep_[FA_N_KEEP] = {nullptr};
	int64_t keep_bytes_[FA_N_KEEP] = {0};
	~SimDrv()
	{
		for (void *p : work_) free(p);
		for (void *p : keep_) free(p);
	}
	template <class F> void items(const char *, int64_t n, const F &f)
	{
		if (rev) for (int64_t i = n - 1; i >= 0; --i) f(i);
		else for (int64_t i = 0; i < n; ++i) f(i);
	}
	void scan(const int64_t *in, int64_t *out, int64_t n) { int64_t a = 0; for (int64_t i = 0; i < n; ++i) { out[i] = a; a += in[i]; } out[n] = a; }
	void scanmax32(int32_t *a, int64_t n) { for (int64_t i = 1; i < n; ++i) a[i] = a[i] > a[i - 1] ? a[i] : a[i - 1]; }
	uint64_t sum64(const uint64_t *in, int64_t n) { uint64_t s = 0; for (int64_t i = 0; i < n; ++i) s += in[i]; return s; }
	int64_t get(const int64_t *p) { return *p; }
	int32_t get32(const int32_t *p) { return *p; }
	void fetch(void *host, const void *dev, size_t bytes) { if (bytes) memcpy(host, dev, bytes); }
	void *work(int slot, int64_t bytes) { free(work_[slot]); work_[slot] = exact(bytes); return work_[slot]; }
	void *keep(int which, int64_t bytes, int64_t kept)
	{
		if (keep_[which] && bytes == keep_bytes_[which]) return keep_[which];
		void *p = exact(bytes);
		const int64_t k = kept < keep_bytes_[which] ? kept : keep_bytes_[which];
		if (keep_[which] && k > 0) memcpy(p, keep_[which], (size_t)(k < bytes ? k : bytes));
		free(keep_[which]);
		keep_[which] = p; keep_bytes_[which] = bytes;
		return p;
	}
};

struct Result {
	int status = 0;
	FaState S;
	std::vector<FaContig> contigs;
	std::vector<FaHole> holes;
	std::vector<uint8_t> pac;
	bool header_cut = false, codes_carried = false;
};

static std::vector<uint8_t> slurp(const std::string &path, bool must = true)
{
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) { if (must) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); } return std::vector<uint8_t>(); }
	std::vector<uint8_t> v;
	uint8_t buf[65536];
	for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
	fclose(f);
	return v;
}

static Result run(const std::vector<uint8_t> &text, int64_t window, bool rev)
{
	Result r;
	SimDrv drv; drv.rev = rev;
	const int64_t n = (int64_t)text.size();
	for (int64_t a = 0; a < n; a += window) {
		const int64_t k = n - a < window ? n - a : window;
		uint8_t *t = (uint8_t *)drv.work(FA_W_TEXT, k);
		memcpy(t, text.data() + a, (size_t)k);
		if (fa_window(drv, r.S, t, k) != FA_OK) { fprintf(stderr, "too many contigs or holes\n"); exit(2); }
		if (a + k < n && r.S.in_hdr) r.header_cut = true;
		if (a + k < n && r.S.n_codes) r.codes_carried = true;
	}
	fa_finish(drv, r.S, r.contigs, r.holes);
	r.status = r.S.bad_start ? 1 : r.S.l_pac == 0 ? 2 : 0;
	if (r.S.contig_too_long) { fprintf(stderr, "a contig too long\n"); exit(2); }
	r.pac.assign((size_t)r.S.pac_bytes(), 0);
	if (!r.pac.empty()) memcpy(r.pac.data(), drv.keep(FA_K_PAC, r.S.pac_bytes(), r.S.pac_bytes()), r.pac.size());
	return r;
}

static bool same(const Result &a, const Result &b)
{
	if (a.status != b.status) return false;
	if (a.status != 0) return true; // refused alike: how far each got is its window's business
	const FaState &x = a.S, &y = b.S;
	if (x.l_pac != y.l_pac || x.n_amb != y.n_amb || x.n_holes != y.n_holes || x.n_contigs != y.n_contigs || x.file_off != y.file_off || memcmp(x.cnt, y.cnt, sizeof x.cnt) ||
	    x.headers != y.headers || a.pac != b.pac || a.contigs.size() != b.contigs.size() || a.holes.size() != b.holes.size())
		return false;
	for (size_t c = 0; c < a.contigs.size(); ++c) {
		const FaContig &p = a.contigs[c], &q = b.contigs[c];
		if (p.hdr_b != q.hdr_b || p.hdr_e != q.hdr_e || p.off != q.off || p.len != q.len || p.n_holes != q.n_holes) return false;
	}
	for (size_t h = 0; h < a.holes.size(); ++h) {
		const FaHole &p = a.holes[h], &q = b.holes[h];
		if (p.off != q.off || p.len != q.len || p.ch != q.ch) return false;
	}
	return true;
}

static std::string no_sort(const uint8_t *, size_t, int64_t, const uint64_t[4], const std::string &) { return ""; }

int main(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: fasta_pack_sim MANIFEST OUTDIR\n"); return 2; }
	for (int b = 0; b < 256; ++b) // the table as arithmetic is the table
		if (fa_code((uint8_t)b) != kNt4[b]) { fprintf(stderr, "fa_code(%d) is not nst_nt4_table's\n", b); return 6; }
	{
		Rand48 r(11); // the jumped generator is the stepped one
		for (uint64_t k = 1; k <= 5000; ++k) {
			const uint32_t v = r.lrand();
			if ((uint32_t)(fa_rand_at(k) >> 17) != v || (k > 1 && fa_rand_step(fa_rand_at(k - 1)) != fa_rand_at(k))) { fprintf(stderr, "fa_rand_at(%llu) is not lrand48's\n", (unsigned long long)k); return 6; }
		}
	}
	FILE *mf = fopen(argv[1], "r");
	if (!mf) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
	char line[4096];
	while (fgets(line, sizeof line, mf)) {
		std::istringstream ls(line);
		std::string name, path, claims;
		int want_status = 0;
		if (!(ls >> name >> path >> want_status >> claims)) continue;
		const std::vector<uint8_t> text = slurp(path);
		const bool skew = ("," + claims + ",").find(",skew,") != std::string::npos;
		Result first;
		bool have = false, many_windows = false, header_cut = false, codes_carried = false;
		int k = 0;
		for (int64_t window : {(int64_t)64, (int64_t)256, (int64_t)4096})
			for (int rev = 0; rev < 2; ++rev, ++k) {
				Result r = run(text, window, rev != 0);
				if (window == 64) { many_windows = many_windows || r.S.windows > 1; header_cut = header_cut || r.header_cut; codes_carried = codes_carried || r.codes_carried; }
				if (skew && k == 3 && !r.pac.empty()) r.pac[0] ^= 0x40;
				if (!have) { first = std::move(r); have = true; continue; }
				if (!same(r, first)) {
					fprintf(stderr, "%s: window %lld rev %d disagrees with the first run (status %d / %d, l_pac %lld / %lld)\n", name.c_str(), (long long)window, rev, r.status, first.status,
					        (long long)r.S.l_pac, (long long)first.S.l_pac);
					return 3;
				}
			}
		std::istringstream cs(claims);
		for (std::string c; std::getline(cs, c, ',');) {
			bool ok = true;
			if (c == "windows") ok = many_windows;
			else if (c == "header") ok = header_cut;
			else if (c == "codes") ok = codes_carried;
			else if (c != "-" && c != "skew") { fprintf(stderr, "%s: unknown claim %s\n", name.c_str(), c.c_str()); return 2; }
			if (!ok) { fprintf(stderr, "%s does not meet its claim: %s\n", name.c_str(), c.c_str()); return 4; }
		}
		if (first.status != want_status) { fprintf(stderr, "%s: status %d, the restatement's is %d\n", name.c_str(), first.status, want_status); return 5; }
		// build_index on the same file
		const std::string prefix = std::string(argv[2]) + "/" + name, host = prefix + ".host";
		const std::string e = build_index(path, host, no_sort);
		const int host_status = e.empty() ? 0 : e == "FASTA does not start with '>'" ? 1 : e == "empty FASTA" ? 2 : -1;
		if (host_status != first.status) { fprintf(stderr, "%s: status %d, build_index says \"%s\"\n", name.c_str(), first.status, e.c_str()); return 6; }
		const FaState &S = first.S;
		printf("case %s %d %lld %lld %lld %lld %llu %llu %llu %llu\n", name.c_str(), first.status, (long long)S.l_pac, (long long)S.n_contigs, (long long)S.n_holes, (long long)S.n_amb,
		       (unsigned long long)S.cnt[0], (unsigned long long)S.cnt[1], (unsigned long long)S.cnt[2], (unsigned long long)S.cnt[3]);
		if (first.status != 0) continue;
		for (const FaContig &c : first.contigs) printf("contig %lld %lld %lld %d %d\n", (long long)c.hdr_b, (long long)c.hdr_e, (long long)c.off, c.len, c.n_holes);
		for (const FaHole &h : first.holes) printf("hole %lld %d %d\n", (long long)h.off, h.len, h.ch);
		// the three files, through the writers the builders share
		{
			FILE *o = fopen((prefix + ".pac").c_str(), "wb");
			if (!o) { fprintf(stderr, "cannot write %s.pac\n", prefix.c_str()); return 2; }
			if (!first.pac.empty()) fwrite(first.pac.data(), 1, first.pac.size(), o);
			fa_write_pac_end(o, S.l_pac);
			fclose(o);
			std::vector<FaAnn> anns;
			std::vector<FaAmb> ambs;
			for (size_t c = 0; c < first.contigs.size(); ++c) {
				FaAnn a = fa_ann_of_header(S.headers[c], first.contigs[c].off);
				a.len = first.contigs[c].len; a.n_ambs = first.contigs[c].n_holes;
				anns.push_back(a);
			}
			for (const FaHole &h : first.holes) ambs.push_back(FaAmb{h.off, h.len, (char)h.ch});
			const std::string we = fa_write_ann_amb(prefix, "", S.l_pac, anns, ambs);
			if (!we.empty()) { fprintf(stderr, "%s\n", we.c_str()); return 2; }
		}
		for (const char *ext : {".pac", ".ann", ".amb"}) {
			const std::vector<uint8_t> ours = slurp(prefix + ext);
			if (ours != slurp(path + ".want" + ext)) { fprintf(stderr, "%s%s differs from the restatement's\n", name.c_str(), ext); return 5; }
			if (ours != slurp(host + ext)) { fprintf(stderr, "%s%s differs from build_index's\n", name.c_str(), ext); return 6; }
		}
		uint64_t sum = 0;
		for (int c = 0; c < 4; ++c) sum += S.cnt[c];
		if (sum != (uint64_t)S.l_pac) { fprintf(stderr, "%s: cnt_fwd sums to %llu of %lld bases\n", name.c_str(), (unsigned long long)sum, (long long)S.l_pac); return 3; }
	}
	fclose(mf);
	return 0;
}

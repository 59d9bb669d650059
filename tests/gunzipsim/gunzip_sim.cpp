// tests/gunzipsim/gunzip_sim.cpp -- TEST PROGRAM, not part of the product: arachne_amd/csrc/dev_gunzip.h and the reader of gunzip_host.h compiled
// for the host.  The lanes of a wavefront run one after the other in a loop, a phase's hand-off is the end of that loop, and the wavefronts of a
// launch run one after the other too.  tests/test_gunzip_sim.py builds it with -fsanitize=address,undefined and runs it as a plain process.
//
//   gunzip_sim IN OUT CHUNK SLAB EXPAND [rev]   IN: a file; it goes through GzReader with the given sizes (0: the defaults) and through zlib's
//                                               gzread.  OUT: the reader's bytes.  Prints "rc" (0: read, 1: an error) and the 13 counts of
//                                               the statistics.  Exit status 3 where the two disagree in bytes or in whether they report an
//                                               error.  rev: lanes and wavefronts run in descending order.
// Every buffer of a launch has exactly the size the kernels are given: an access past any of them is the sanitizer's to find.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <zlib.h>
#include "../../arachne_amd/csrc/gunzip_host.h"

using namespace arx;

struct SimDrv {
	bool rev = false;
	template <class F> void lanes(F f)
	{
		if (rev) for (int l = INF_LANES - 1; l >= 0; --l) f(l);
		else for (int l = 0; l < INF_LANES; ++l) f(l);
	}
};

struct SimBackend {
	bool rev = false;
	template <class F> void each(int n, F f)
	{
		if (rev) for (int k = n - 1; k >= 0; --k) f(k);
		else for (int k = 0; k < n; ++k) f(k);
	}
	std::vector<uint16_t> stage;
	std::vector<uint8_t> windows;
	void decode(const uint8_t *src_, int clen, int start_bit, const uint8_t *window, int have, int chunk_bytes, int expand, GzLaunch &L)
	{
		const int n = (int)(((int64_t)clen + chunk_bytes - 1) / chunk_bytes);
		const std::vector<uint8_t> src(src_, src_ + clen);
		stage.assign((size_t)gz_stage_at(8 * (int64_t)clen, expand), 0xA5A5);
		windows.assign((size_t)(n + 1) * GZ_WIN, 0xA5);
		memcpy(windows.data(), window, GZ_WIN);
		std::vector<uint32_t> mem(GZ_WORK_BYTES / 4);
		L.chunks.assign((size_t)n, GzChunk());
		SimDrv drv; drv.rev = rev;
		GzWork w;
		gz_carve(w, (uint8_t *)mem.data());
		each(n, [&](int k) {
			memset(mem.data(), 0x5A, mem.size() * 4); // dirty work memory: nothing may depend on what the chunk before left
			gz_chunk_find(drv, w, src.data(), clen, chunk_bytes, start_bit, k, L.chunks[(size_t)k]);
		});
		each(n, [&](int k) {
			memset(mem.data(), 0x5A, mem.size() * 4);
			gz_chunk_decode(drv, w, src.data(), clen, expand, k, n, L.chunks.data(), stage.data());
		});
		gz_chain(L.chunks.data(), n, have, L.chain);
		for (int m = 0, k = 0; m < L.chain.n_accepted; ++m) {
			GzChunk &c = L.chunks[(size_t)k];
			if (c.have < GZ_WIN) each(c.count, [&](int i) { c.bad_markers += gz_bad_marker_at(stage.data() + c.stage_off, c.have, i); });
			each(GZ_WIN, [&](int i) { gz_window_at(windows.data() + (size_t)m * GZ_WIN, windows.data() + (size_t)(m + 1) * GZ_WIN, stage.data() + c.stage_off, c.count, i); });
			k = c.next;
		}
		for (double &u : L.us) u = 0;
	}
	void resolve(GzLaunch &L, uint8_t *text_)
	{
		const int n = (int)L.chunks.size();
		std::vector<uint8_t> all((size_t)L.chain.text_bytes, 0xA5); // exactly the bytes of the piece
		uint32_t crc_tab[256], x2n[32];
		each(64, [&](int lane) { gz_crc_tables(crc_tab, x2n, lane, 64); });
		each(n, [&](int k) {
			GzChunk &c = L.chunks[(size_t)k];
			if (!(c.flags & GZ_F_ACCEPTED)) return;
			uint8_t *text = all.data() + c.text_off;
			each(c.count, [&](int i) { c.markers += gz_resolve_at(windows.data() + (size_t)c.order * GZ_WIN, stage.data() + c.stage_off, text, i); });
			const int T = 256;
			c.crc = 0;
			each(T, [&](int t) { c.crc ^= gz_crc_part(crc_tab, x2n, text, c.count, t, T); });
		});
		if (!all.empty()) memcpy(text_, all.data(), all.size());
		memcpy(L.window, windows.data() + (size_t)L.chain.n_accepted * GZ_WIN, GZ_WIN);
	}
	void upload(uint8_t *dst, const uint8_t *host, size_t bytes) { if (bytes) memcpy(dst, host, bytes); }
};

// gzread of the whole file; -> false: it reports an error
static bool by_gzread(const char *path, std::vector<uint8_t> &out)
{
	gzFile g = gzopen(path, "rb");
	if (!g) return false;
	std::vector<uint8_t> b(1 << 16);
	bool ok = true;
	for (;;) {
		const int k = gzread(g, b.data(), (unsigned)b.size());
		if (k < 0) { ok = false; break; }
		if (k == 0) break;
		out.insert(out.end(), b.begin(), b.begin() + k);
	}
	int err = 0;
	gzerror(g, &err);
	if (err != Z_OK && err != Z_STREAM_END) ok = false;
	gzclose(g);
	return ok;
}

int main(int argc, char **argv)
{
	if (argc < 6) { fprintf(stderr, "usage: gunzip_sim IN OUT CHUNK SLAB EXPAND [rev]\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
	std::vector<uint8_t> in;
	uint8_t b[65536];
	for (size_t k; (k = fread(b, 1, sizeof b, f)) > 0;) in.insert(in.end(), b, b + k);
	fclose(f);
	const int64_t chunk = atoll(argv[3]) ? atoll(argv[3]) : GZ_CHUNK_DEFAULT, slab = atoll(argv[4]) ? atoll(argv[4]) : GZ_SLAB_DEFAULT;
	const int32_t expand = atoi(argv[5]) ? atoi(argv[5]) : GZ_EXPAND_DEFAULT;
	if (chunk < GZ_MIN_CHUNK || slab < 2 * chunk || slab > GZ_MAX_SLAB || slab > GZ_MAX_CHUNKS * chunk || expand < 1 || expand > GZ_MAX_EXPAND || slab * expand > GZ_MAX_SYMBOLS) { fprintf(stderr, "sizes outside their bounds\n"); return 2; }
	SimBackend dev; dev.rev = argc > 6 && !strcmp(argv[6], "rev");
	const std::vector<uint8_t> exact(in); // an allocation of exactly the file's bytes
	GzMemSource src(exact.data(), (int64_t)exact.size());
	GzReader<SimBackend> r(dev, src, chunk, slab, expand);
	r.can_rewind = true;
	std::vector<uint8_t> got;
	bool ok = true;
	for (;;) {
		const int64_t k = r.next();
		if (k == GZ_END) break;
		if (k == GZ_ERROR) { ok = false; break; }
		if (k == GZ_REWIND) { got.resize((size_t)r.rewind_to); continue; }
		std::vector<uint8_t> piece((size_t)k, 0xA5); // a place of exactly the piece's bytes
		r.place(piece.data());
		got.insert(got.end(), piece.begin(), piece.end());
	}
	std::vector<uint8_t> want;
	const bool want_ok = by_gzread(argv[1], want);
	if (ok != want_ok) { fprintf(stderr, "the reader %s, gzread %s\n", ok ? "reads it" : "reports an error", want_ok ? "reads it" : "reports an error"); return 3; }
	if (ok && (got.size() != want.size() || (!want.empty() && memcmp(got.data(), want.data(), want.size())))) {
		fprintf(stderr, "the reader's %zu bytes are not gzread's %zu\n", got.size(), want.size());
		return 3;
	}
	FILE *o = fopen(argv[2], "wb");
	if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
	if (ok && !got.empty()) fwrite(got.data(), 1, got.size(), o);
	fclose(o);
	printf("%d", ok ? 0 : 1);
	for (int k = 0; k < 13; ++k) printf(" %lld", (long long)r.stats[k]);
	printf("\n");
	return 0;
}

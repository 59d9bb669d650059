// gunzip_host.h -- the host side of the chunked gzip inflate (dev_gunzip.h): plain C++ and zlib, no HIP, so that the host twin
// (tests/gunzipsim/gunzip_sim.cpp) compiles the very same reader with the device logic run in a loop behind it.
//
// GzReader<Backend> turns a gzip file into its bytes the way zlib's gzread does, a piece at a time: next() says how many bytes the next piece
// has, place(dst) puts them where the caller wants them (for a piece the device decoded that is the resolve phase itself: the text is written
// once, at its final place).  The framing is done here, on the calling thread: member headers (FEXTRA, FNAME, FCOMMENT, FHCRC with its CRC-16,
// the reserved flag bits), trailers, the running CRC-32 and length of a member (the chunks' CRCs put together with crc32_combine), the next
// member, and gzread's rule for what follows the last one: bytes that do not start with the gzip magic are ignored.  The DEFLATE body goes to
// the backend a slab at a time (Backend::decode: the phases of dev_gunzip.h up to the windows; Backend::resolve: the last one); the bytes of a
// slab behind the accepted chain are carried into the next launch, not read again.
//
// The yardstick is gzread: for every input it reads without error the bytes are its bytes; for every input on which it reports an error the
// result is an error.  So that this holds without restating zlib's judgement the device never declares a file bad.  Whatever it does not take
// -- a refuted candidate, an overflow of a staging span, a status other than OK where the chain stops, a marker in front of the member's
// start, a CRC or length that does not match the trailer, a slab in which no block ends, two launches in a row cut to less than a quarter of
// their bytes by member ends -- hands the rest of the file to the host: a raw zlib inflate primed with the carried bit and window
// (inflatePrime, inflateSetDictionary), followed by the same framing code.  What zlib and the trailer then say decides.  A member whose
// trailer does not match what the device produced is read again from its header by the host where the source can go back and the caller can
// drop the member's bytes (GZ_REWIND; the self-test); a caller that has passed them on gets an error instead (the file calls).
//
// A backend may offer its two calls in halves (decode_begin / decode_end, resolve_begin / resolve_end: hip_gunzip.h's GzHip does): begin() and
// place_begin() then enqueue what next() and place() would start and only wait for, so that a caller with several files (device_feeder.h) has
// every file's launch in flight before it waits for any.  Without the halves they do nothing, and without a call of them nothing changes.
//
// Out of scope: decoding on from a member end inside the same launch (the launch behind a member end starts behind the trailer and the next
// header, with an empty window), fixed or stored blocks as chunk starts.
#pragma once
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include <utility>
#include <vector>
#include <zlib.h>
#include "dev_gunzip.h"

namespace arx {

// the defaults of a reader.  The chunk: the fastest of 32 / 64 / 128 KiB on level-1 FASTQ (profiles/device_gunzip/README.md); the slab and the
// expansion were not swept
constexpr int64_t GZ_CHUNK_DEFAULT = 32 << 10, GZ_SLAB_DEFAULT = 8 << 20, GZ_MIN_CHUNK = 64;
constexpr int32_t GZ_EXPAND_DEFAULT = 8, GZ_MAX_EXPAND = 1032; // (DEFLATE's own limit is 1032 bytes per compressed byte)
constexpr size_t GZ_HOST_PIECE = 4 << 20;                      // bytes of a piece the host inflates

enum { GZ_FB_NONE = 0, GZ_FB_REFUTED, GZ_FB_OVERFLOW, GZ_FB_STATUS, GZ_FB_CHECK, GZ_FB_NO_BLOCK, GZ_FB_CUT_SHORT }; // why the host took over
enum { GZS_MEMBERS = 0, GZS_CONSUMED, GZS_INFLATED, GZS_LAUNCHES, GZS_CHUNKS, GZS_CANDIDATES, GZS_ACCEPTED, GZS_REFUTED, GZS_BLOCKS, GZS_MARKERS, GZS_HOST_BYTES, GZS_REASON,
       GZS_IGNORED, GZS_US_FIND, GZS_US_DECODE, GZS_US_RESOLVE, GZ_N_STATS }; // (GZS_US_RESOLVE: the windows and the resolve)
static_assert(GZ_N_STATS == 16, "arx_selftest_gunzip's stats");
enum { GZ_END = -1, GZ_ERROR = -2, GZ_REWIND = -3 }; // GzReader::next()

// what a launch hands back
struct GzLaunch {
	std::vector<GzChunk> chunks;
	GzChain chain;
	uint8_t window[GZ_WIN]; // the window behind the last accepted chunk (after resolve)
	double us[4];           // find, decode, windows, resolve
};

// the compressed bytes: read in order, and from an earlier place again where a member is handed to the host
struct GzSource {
	virtual size_t read(uint8_t *to, size_t n) = 0;
	virtual bool seek(int64_t) { return false; }
	virtual ~GzSource() {}
};
struct GzMemSource : GzSource {
	const uint8_t *p; int64_t n, at = 0;
	GzMemSource(const uint8_t *p_, int64_t n_) : p(p_), n(n_) {}
	size_t read(uint8_t *to, size_t k) override
	{
		const size_t got = (int64_t)k < n - at ? k : (size_t)(n - at);
		if (got) memcpy(to, p + at, got);
		at += (int64_t)got;
		return got;
	}
	bool seek(int64_t to) override { if (to < 0 || to > n) return false; at = to; return true; }
};

template <class B, class = void> struct gz_has_halves : std::false_type {};
template <class B> struct gz_has_halves<B, std::void_t<decltype(&B::decode_begin), decltype(&B::decode_end), decltype(&B::resolve_begin), decltype(&B::resolve_end)> > : std::true_type {};

template <class Backend> struct GzReader {
	static constexpr bool HALVES = gz_has_halves<Backend>::value;
	Backend &dev;
	GzSource &src;
	int64_t chunk_bytes, slab_bytes; int32_t expand;
	bool can_rewind = false;  // the caller drops a member's bytes on GZ_REWIND
	std::vector<uint8_t> buf; // compressed bytes read and not yet consumed
	int64_t buf_at = 0;       // where buf[0] lies in the file
	bool eof = false, host = false, first = true;
	int n_short = 0;
	int64_t stats[GZ_N_STATS];
	double us[4] = {0, 0, 0, 0};
	GzLaunch L;
	enum { S_LOOK, S_BODY, S_TRAILER, S_COPY, S_END } state = S_LOOK;
	// the member that is being read
	int64_t member_at = 0, member_out = 0;
	bool by_device = false, again = false;
	uint8_t window[GZ_WIN];
	int bit = 0, have = 0;
	uLong crc = 0;
	uint64_t len = 0;
	z_stream z;
	bool z_open = false;
	// the piece next() announced
	int piece = 0; // 1: the device's (L), 2: the host's (host_piece)
	int64_t piece_n = 0, launch_n = 0;
	std::vector<uint8_t> host_piece;
	int64_t delivered = 0, rewind_to = 0;
	// the halves: a launch that begin() enqueued, what begin() met instead of one, a resolve that place_begin() enqueued
	bool launched = false, held = false, resolving = false;
	int64_t held_value = 0;

	GzReader(Backend &dev_, GzSource &src_, int64_t chunk, int64_t slab, int32_t expand_) : dev(dev_), src(src_), chunk_bytes(chunk), slab_bytes(slab), expand(expand_)
	{
		for (int64_t &s : stats) s = 0;
	}
	~GzReader() { if (z_open) inflateEnd(&z); }
	GzReader(const GzReader &) = delete;

	// buf holds at least n bytes, or all there are
	void fill(size_t n)
	{
		while (!eof && buf.size() < n) {
			const size_t had = buf.size(), want = n - had;
			buf.resize(n);
			const size_t got = src.read(buf.data() + had, want);
			buf.resize(had + got);
			if (got < want) eof = true;
		}
	}
	void consume(size_t n) { buf.erase(buf.begin(), buf.begin() + (ptrdiff_t)n); buf_at += (int64_t)n; }
	void to_host(int reason) { host = true; if (!stats[GZS_REASON]) stats[GZS_REASON] = reason; }

	// the member header at buf[0]; -> its length, 0: gzread reports an error
	size_t header()
	{
		fill(10);
		if (buf.size() < 10 || buf[2] != 8 || (buf[3] & 0xE0)) return 0;
		const int flg = buf[3];
		size_t at = 10;
		if (flg & 4) {
			fill(at + 2);
			if (buf.size() < at + 2) return 0;
			at += 2 + (size_t)(buf[at] | buf[at + 1] << 8);
			fill(at);
			if (buf.size() < at) return 0;
		}
		for (int fb = 8; fb <= 16; fb <<= 1) { // FNAME, FCOMMENT: to their zero
			if (!(flg & fb)) continue;
			for (;; ++at) {
				if (at >= buf.size()) { fill(buf.size() + 4096); if (at >= buf.size()) return 0; }
				if (!buf[at]) break;
			}
			++at;
		}
		if (flg & 2) {
			fill(at + 2);
			if (buf.size() < at + 2) return 0;
			if ((crc32(0L, buf.data(), (uInt)at) & 0xFFFFu) != (uLong)(buf[at] | buf[at + 1] << 8)) return 0;
			at += 2;
		}
		return at;
	}
	bool begin_member()
	{
		const size_t hdr = header();
		if (!hdr) return false;
		consume(hdr);
		memset(window, 0, sizeof window);
		bit = 0; have = 0; len = 0; by_device = false;
		crc = crc32(0L, Z_NULL, 0);
		state = S_BODY;
		return true;
	}

	// The next bytes of the member's body by zlib, from bit `bit` of buf[0] with the carried window at first; at most GZ_HOST_PIECE of them into
	// host_piece.  false: zlib reports an error or the bytes end.  Behind the last block buf stands at the trailer
	bool host_step()
	{
		if (!z_open) {
			memset(&z, 0, sizeof z);
			if (inflateInit2(&z, -15) != Z_OK) return false;
			z_open = true;
			fill(1);
			if (bit > 0) {
				if (buf.empty() || inflatePrime(&z, 8 - bit, buf[0] >> bit) != Z_OK) return false;
				consume(1);
				bit = 0;
			}
			if (have > 0 && inflateSetDictionary(&z, window + GZ_WIN - have, (uInt)have) != Z_OK) return false;
		}
		host_piece.resize(GZ_HOST_PIECE);
		size_t made = 0;
		bool done = false;
		while (!done && made < host_piece.size()) {
			fill((size_t)slab_bytes);
			if (buf.empty()) return false; // zlib would be asked with nothing: gzread calls that an unexpected end of file
			z.next_in = buf.data(); z.avail_in = (uInt)buf.size();
			z.next_out = host_piece.data() + made; z.avail_out = (uInt)(host_piece.size() - made);
			const int r = inflate(&z, Z_NO_FLUSH);
			made = host_piece.size() - z.avail_out;
			const size_t used = buf.size() - z.avail_in;
			consume(used);
			if (r == Z_STREAM_END) done = true;
			else if (r == Z_BUF_ERROR) { if (used == 0 && eof && z.avail_out) return false; } // nothing more to give it
			else if (r != Z_OK) return false;
		}
		host_piece.resize(made);
		if (made) { crc = crc32(crc, host_piece.data(), (uInt)made); len += made; stats[GZS_HOST_BYTES] += (int64_t)made; }
		if (done) { inflateEnd(&z); z_open = false; state = S_TRAILER; }
		return true;
	}

	// One launch on the bytes in buf, up to the windows.  -> true: a chain was accepted and awaits its resolve (accept()); false: the device did
	// not take it, and `host` is set
	bool device_step(bool begin_only = false)
	{
		if (!launched) {
			if (n_short >= 2) { to_host(GZ_FB_CUT_SHORT); return false; } // two such launches in a row: whatever follows is the host's
			fill((size_t)slab_bytes);
			const int64_t n = (int64_t)buf.size() < slab_bytes ? (int64_t)buf.size() : slab_bytes;
			if (n == 0 || bit >= 8 * n) { to_host(GZ_FB_NO_BLOCK); return false; }
			launch_n = n;
			if constexpr (HALVES) {
				dev.decode_begin(buf.data(), (int)n, bit, window, have, (int)chunk_bytes, expand); // (buf, bit and window stay as they are until decode_end)
				launched = true;
				if (begin_only) return true;
			} else dev.decode(buf.data(), (int)n, bit, window, have, (int)chunk_bytes, expand, L);
		}
		if constexpr (HALVES) { launched = false; dev.decode_end(L); }
		const int64_t n = launch_n;
		++stats[GZS_LAUNCHES]; stats[GZS_CHUNKS] += (int64_t)L.chunks.size();
		for (int p = 0; p < 3; ++p) us[p] += L.us[p];
		const int nc = (int)L.chunks.size();
		for (const GzChunk &c : L.chunks) stats[GZS_CANDIDATES] += c.cand >= 0;
		bool sound = nc > 0 && L.chain.n_accepted > 0 && L.chain.last >= 0 && L.chain.last < nc;
		if (sound) { // the chain as the device walked it, checked as it is read
			int64_t total = 0;
			int m = 0;
			for (int k = 0; k < nc && m < L.chain.n_accepted; ++m) {
				const GzChunk &c = L.chunks[(size_t)k];
				if (!(c.flags & GZ_F_ACCEPTED) || c.order != m || c.text_off != total || c.count < 0 || c.bad_markers) { sound = false; break; }
				total += c.count;
				if (m + 1 < L.chain.n_accepted && (c.next <= k || c.next >= nc)) { sound = false; break; }
				if (m + 1 == L.chain.n_accepted && k != L.chain.last) { sound = false; break; }
				k = c.next;
			}
			const GzChunk &last = L.chunks[(size_t)L.chain.last];
			if (m != L.chain.n_accepted || total != L.chain.text_bytes || last.end_bit < bit || last.end_bit > 8 * n) sound = false;
		}
		if (!sound) {
			const int st0 = nc > 0 ? L.chunks[0].status : GZ_BAD_STREAM;
			to_host(L.chain.n_accepted > 0 ? GZ_FB_STATUS : st0 == GZ_OVERFLOW ? GZ_FB_OVERFLOW : st0 == GZ_NO_BLOCK ? GZ_FB_NO_BLOCK : GZ_FB_STATUS);
			return false;
		}
		by_device = true;
		return true;
	}
	// behind the resolve of an accepted chain: the member's CRC and length, the window, and buf and bit moved behind what was accepted
	void accept()
	{
		const int nc = (int)L.chunks.size();
		for (int k = 0, m = 0; m < L.chain.n_accepted; ++m) {
			const GzChunk &c = L.chunks[(size_t)k];
			crc = crc32_combine(crc, c.crc, (z_off_t)c.count);
			len += (uint64_t)c.count;
			stats[GZS_BLOCKS] += c.blocks; stats[GZS_MARKERS] += c.markers;
			k = c.next;
		}
		stats[GZS_ACCEPTED] += L.chain.n_accepted;
		us[3] += L.us[3];
		memcpy(window, L.window, GZ_WIN);
		have = L.chain.have;
		const GzChunk &last = L.chunks[(size_t)L.chain.last];
		const bool ended = (last.flags & GZ_F_MEMBER_END) != 0;
		int reason = GZ_FB_NONE;
		if (!ended) {
			if (last.flags & GZ_F_PASSED) { reason = GZ_FB_REFUTED; ++stats[GZS_REFUTED]; }
			else if ((last.flags & GZ_F_CONFIRMED) && last.next < nc) { // where the chain stopped: on a true block start the device did not take
				const GzChunk &nx = L.chunks[(size_t)last.next];
				if (nx.status == GZ_OVERFLOW) reason = GZ_FB_OVERFLOW;
				else if (nx.status == GZ_BAD_STREAM) reason = GZ_FB_STATUS;
			}
		}
		n_short = ended && (int64_t)last.end_bit * 4 < 8 * launch_n ? n_short + 1 : 0; // cut to less than a quarter of its bytes by a member end
		consume((size_t)(last.end_bit >> 3));
		bit = last.end_bit & 7;
		if (reason) to_host(reason);
		if (ended) state = S_TRAILER;
	}
	void finish()
	{
		stats[GZS_CONSUMED] = buf_at - stats[GZS_IGNORED];
		stats[GZS_INFLATED] = delivered;
		stats[GZS_US_FIND] = (int64_t)us[0]; stats[GZS_US_DECODE] = (int64_t)us[1]; stats[GZS_US_RESOLVE] = (int64_t)(us[2] + us[3]);
		state = S_END;
	}

	// -> the bytes of the next piece (more than none; place() puts them somewhere), GZ_END behind the last one, GZ_ERROR where gzread reports
	// an error, GZ_REWIND (can_rewind only): the bytes delivered behind the first rewind_to are dropped, the reading goes on
	int64_t next()
	{
		if (held) { held = false; return held_value; }
		return run(false);
	}
	// the enqueue half of next(): where the next piece is the device's its launch is started and next() waits for it; anything else next()
	// would have met on the way (a piece of the host's, the end, an error) is kept for it
	void begin()
	{
		if (!HALVES || held || launched || piece) return;
		const int64_t r = run(true);
		if (!launched) { held = true; held_value = r; }
	}
	int64_t run(bool begin_only)
	{
		for (;;) {
			if (state == S_END) return GZ_END;
			if (state == S_COPY) { // no gzip file: gzread hands the bytes on as they are
				fill((size_t)slab_bytes);
				if (buf.empty()) { finish(); continue; }
				host_piece.assign(buf.begin(), buf.end());
				consume(buf.size());
				piece = 2;
				return piece_n = (int64_t)host_piece.size();
			}
			if (state == S_LOOK) {
				fill(2);
				if (buf.empty()) { finish(); continue; }
				if (buf.size() < 2 || buf[0] != 0x1F || buf[1] != 0x8B) {
					if (first) { state = S_COPY; continue; }
					do { stats[GZS_IGNORED] += (int64_t)buf.size(); consume(buf.size()); fill((size_t)slab_bytes); } while (!buf.empty());
					finish();
					continue;
				}
				first = false; again = false;
				member_at = buf_at; member_out = delivered;
				if (!begin_member()) return GZ_ERROR;
				continue;
			}
			if (state == S_BODY) {
				if (host) {
					if (!host_step()) return GZ_ERROR;
					if (host_piece.empty()) continue;
					piece = 2;
					return piece_n = (int64_t)host_piece.size();
				}
				if (begin_only && !launched) { if (!device_step(true)) continue; return 0; }
				if (!device_step()) continue;
				if (L.chain.text_bytes == 0) { dev.resolve(L, nullptr); accept(); continue; } // (the chunks' CRCs of no bytes, and the window)
				piece = 1;
				return piece_n = L.chain.text_bytes;
			}
			// S_TRAILER
			if (bit) { consume(1); bit = 0; } // the trailer starts on a byte
			fill(8);
			if (buf.size() < 8) return GZ_ERROR;
			const uint32_t want_crc = (uint32_t)buf[0] | (uint32_t)buf[1] << 8 | (uint32_t)buf[2] << 16 | (uint32_t)buf[3] << 24;
			const uint32_t want_len = (uint32_t)buf[4] | (uint32_t)buf[5] << 8 | (uint32_t)buf[6] << 16 | (uint32_t)buf[7] << 24;
			if (want_crc == (uint32_t)crc && want_len == (uint32_t)len) { consume(8); ++stats[GZS_MEMBERS]; state = S_LOOK; continue; }
			if (!by_device || again || !can_rewind) return GZ_ERROR; // zlib's bytes do not match the trailer: gzread's error
			// the device's do not: the member again, by the host
			to_host(GZ_FB_CHECK);
			if (!src.seek(member_at)) return GZ_ERROR;
			buf.clear(); buf_at = member_at; eof = false; again = true;
			rewind_to = delivered = member_out;
			if (!begin_member()) return GZ_ERROR;
			return GZ_REWIND;
		}
	}
	// the piece next() announced to dst[0, its bytes): the backend's memory
	// the enqueue half of place(dst) for a piece of the device's: place(dst) then waits for it
	void place_begin(uint8_t *dst)
	{
		if constexpr (HALVES) { if (piece == 1 && !resolving) { dev.resolve_begin(L, dst); resolving = true; } }
		(void)dst;
	}
	void place(uint8_t *dst)
	{
		if (piece == 1) {
			if constexpr (HALVES) { if (!resolving) dev.resolve_begin(L, dst); resolving = false; dev.resolve_end(L); }
			else dev.resolve(L, dst);
			accept();
		}
		else if (piece == 2) dev.upload(dst, host_piece.data(), host_piece.size());
		delivered += piece_n;
		piece = 0; piece_n = 0;
	}
};

} // namespace arx

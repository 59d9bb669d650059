// bgzf_walk.h -- the walk over the headers of a chain of BGZF blocks (the SAM specification, 4.1), and the row that tells the inflate kernel
// (dev_inflate.h, hip_inflate.h) where a block is.  Plain C++ without device code: the reader thread of the device feeder (feeder.h:
// BgzfChunkReader), the self-test entry (arx_selftest_inflate) and the host test program walk with these same functions.
#pragma once
#include <stdint.h>
#include <stddef.h>

namespace arx {

constexpr int INF_MAX_OUT = 65536;  // bytes of a BGZF block, inflated

// One row of a launch's table: where the block's DEFLATE stream is (coff, clen: relative to the launch's compressed base), where its bytes
// go (ooff: relative to the launch's output base), and what its trailer says.  clen < 0: the block's header was refused (INF_BAD_HEADER, dev_inflate.h)
struct InfRow { int64_t coff, ooff; int32_t clen, isize; uint32_t crc; int32_t pad; };

struct BgzfHeader {
	int block;   // bytes of the whole block (BSIZE + 1)
	int payload; // offset of the DEFLATE stream: 12 + XLEN
	bool sound;  // CM is 8, FLG is FEXTRA alone, and the block holds its header and trailer: otherwise the block is INF_BAD_HEADER
};
// p[0, n): the start of a block.  1: *h is filled; 0: n is too small to say (12 + XLEN bytes are needed); -1: not a BGZF header, i.e. no gzip
// magic, no FEXTRA, or no BC subfield of length 2 among the extra subfields (the test htslib makes)
inline int bgzf_read_header(const uint8_t *p, size_t n, BgzfHeader *h)
{
	if (n < 12) return 0;
	if (p[0] != 0x1f || p[1] != 0x8b || !(p[3] & 4)) return -1;
	const size_t xlen = (size_t)p[10] | (size_t)p[11] << 8;
	if (n < 12 + xlen) return 0;
	for (size_t o = 12; o + 4 <= 12 + xlen;) {
		const size_t slen = (size_t)p[o + 2] | (size_t)p[o + 3] << 8;
		if (o + 4 + slen > 12 + xlen) break;
		if (p[o] == 'B' && p[o + 1] == 'C' && slen == 2) {
			h->block = ((int)p[o + 4] | (int)p[o + 5] << 8) + 1;
			h->payload = (int)(12 + xlen);
			h->sound = p[2] == 8 && p[3] == 4 && h->block >= h->payload + 8;
			return 1;
		}
		o += 4 + slen;
	}
	return -1;
}
// the row of the whole block p[0, h.block) that starts at offset `at` of the launch's compressed bytes and whose bytes go to offset `ooff`
inline InfRow bgzf_row(const uint8_t *p, const BgzfHeader &h, int64_t at, int64_t ooff)
{
	InfRow r = {at + h.payload, ooff, -1, 0, 0, 0};
	if (!h.sound) return r;
	const uint8_t *t = p + h.block - 8;
	r.crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
	const uint32_t isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
	if (isize > (uint32_t)INF_MAX_OUT) return r; // clen stays -1
	r.clen = h.block - h.payload - 8; r.isize = (int32_t)isize;
	return r;
}

// the chain src[0, n) -> its rows (at most cap; rows may be null to count only), the output offsets running from 0.  Returns the number of
// blocks, or -1 where the headers do not tile src exactly; *out_bytes: the sum of ISIZE over the sound blocks
inline int64_t bgzf_walk(const uint8_t *src, int64_t n, InfRow *rows, int64_t cap, int64_t *out_bytes)
{
	int64_t nb = 0, total = 0;
	for (int64_t at = 0; at < n; ++nb) {
		BgzfHeader h;
		if (bgzf_read_header(src + at, (size_t)(n - at), &h) != 1 || h.block > n - at) return -1;
		const InfRow r = bgzf_row(src + at, h, at, total);
		if (rows && nb < cap) rows[nb] = r;
		total += r.isize;
		at += h.block;
	}
	*out_bytes = total;
	return nb;
}

} // namespace arx

// dev_fapack.h -- the step that opens every run, on the device: a FASTA text turned into the packed forward strand, the contig table and the hole
// table of the reference's `bwa index` (bntseq.c:227-328 bns_fasta2bntseq), window by window.  The rules are build_index's (index_build.h), to the
// byte; they are not restated differently here, only evaluated in parallel.  As dev_fqstd.h it is launches over an explicit item index, shared by
// the kernels' driver (hip_fapack.h) and the host program (tests/fapacksim/fasta_pack_sim.cpp) through the same `drv`:
//     drv.items(name, n, f)            f(i) for every i in [0, n), in any order
//     drv.scan(in, out, n)             out[0] = 0, out[i + 1] = in[0] + .. + in[i] (int64)
//     drv.scanmax32(a, n)              a[i] = max(a[0] .. a[i]) in place (int32)
//     drv.sum64(in, n)                 the sum (uint64)
//     drv.get / get32 / fetch          values and bytes read home
//     drv.work(slot, bytes)            scratch of a window (FA_W_*): its content does not outlive the window
//     drv.keep(which, bytes, kept)     what lives as long as the call (FA_K_*): grown when `bytes` do not fit, the first `kept` bytes staying
//
// The walk has two states, sequence and header.  Both '>' and '\n' set the state whatever it was ('>' -> header, also inside a header, where it
// changes nothing; '\n' -> sequence), no other byte touches it: the state in front of a 16-byte word is that of the last such byte before it.
// Pass by pass, one item per word of the window (one 16-byte load per item where the word is whole):
//   fa_maps    the last '>' or '\n' of the word as (word + 1) << 1 | state; a running maximum makes it the state in front of every word
//   fa_count   bases, ambiguous bases; the word's last base byte or header end as (word + 1) << 10 | what; the running maximum of that is the
//              base byte in front of every word within its contig (what a hole start is decided by), the sums are where a word's bases go
//   fa_holes   header ends and hole starts of the word (an ambiguous base that opens its contig or follows another base byte); their sums are
//              the word's contig and the ordinal of its holes
//   fa_emit    one code byte per base at its place in the window's code list (behind the 0 .. 63 codes the window before left over), the N's
//              replaced by lrand48() & 3 of the stream srand48(11) at their ordinal in the whole file -- the generator is jumped to the ordinal
//              of a word's first N by the affine maps of 2^j steps and stepped from there --, the hole rows, the contig rows
//   fa_pack    output-stationary: an item owns 16 bytes of .pac (one aligned 16-byte store), reads its 64 codes (four aligned 16-byte loads)
//              and counts them; the sums of the counts are cnt_fwd.  Only whole groups of 64 codes are packed, so that every store of every
//              window is aligned; the rest is carried, and the call's last group is written byte by byte
// No atomics, no item depends on another of its launch.  The carry between windows (FaState) is O(1): the state, the last base byte of the open
// contig, the counts (64-bit), up to 63 codes; the text of a header that a window cuts is joined on the host, and headers are the only text
// that goes there.  The lengths of contigs and holes are differences of neighbouring rows, taken when the input has ended.
#pragma once
#include <string>
#include <vector>
#include "dev_fqsort.h"

namespace arx {

constexpr int64_t FA_MIN_WINDOW = 64;
constexpr int64_t FA_MAX_WINDOW = (int64_t)16 << 20;     // (words + 1) << 10 stays below 2^31
constexpr int64_t FA_WINDOW_DEFAULT = FA_MAX_WINDOW;
enum { FA_OK = 0, FA_E_COUNT = 1 };                      // more than 2^31 - 1 contigs or holes
enum { FA_W_TEXT = 0, FA_W_HMAP, FA_W_EV, FA_W_CNTA, FA_W_OFFA, FA_W_CNTB, FA_W_OFFB, FA_W_CODES, FA_W_PCA, FA_W_PCB, FA_W_META, FA_N_WORK };
static_assert(FA_N_WORK <= FS_N_WORK, "the sort's driver holds the work slots");
enum { FA_K_PAC = 0, FA_K_CONTIGS, FA_K_HOLES, FA_K_CARRY, FA_N_KEEP };
constexpr int32_t FA_EV_START = 0x200, FA_EV_BASE = 0x100; // what stands in front of a base: the start of its contig, or 0x100 | the base byte
constexpr uint64_t FA_RAND_A = 0x5DEECE66DULL, FA_RAND_C = 0xB, FA_RAND_MASK = ((uint64_t)1 << 48) - 1, FA_RAND_X0 = ((uint64_t)11 << 16) | 0x330E;

struct FaContig { int64_t hdr_b, hdr_e, off, hole0; int32_t len, n_holes; }; // header text [hdr_b, hdr_e) of the file; first base; first hole
struct FaHole { int64_t off, aord; int32_t ch, len; };                       // first base; its ordinal among the ambiguous bases; the byte

// nst_nt4_table (bntseq.c:47-64) as arithmetic: A/C/G/T in either case -> 0..3, '-' -> 5, the rest -> 4
ARX_DEVI int fa_code(uint8_t ch)
{
	const uint8_t l = ch | 0x20;
	return l == 'a' ? 0 : l == 'c' ? 1 : l == 'g' ? 2 : l == 't' ? 3 : ch == '-' ? 5 : 4;
}
// X_k of the drand48 family after srand48(11), k >= 0: the affine map of k steps composed from those of 2^j steps, mod 2^48
ARX_DEVI uint64_t fa_rand_at(uint64_t k)
{
	uint64_t a = FA_RAND_A, c = FA_RAND_C, ra = 1, rc = 0;
	for (; k; k >>= 1) {
		if (k & 1) { ra = (a * ra) & FA_RAND_MASK; rc = (a * rc + c) & FA_RAND_MASK; }
		c = (a * c + c) & FA_RAND_MASK; a = (a * a) & FA_RAND_MASK;
	}
	return (ra * FA_RAND_X0 + rc) & FA_RAND_MASK;
}
ARX_DEVI uint64_t fa_rand_step(uint64_t x) { return (FA_RAND_A * x + FA_RAND_C) & FA_RAND_MASK; }

// the bytes of word w of t[0, n) -> how many there are
ARX_DEVI int fa_load(const uint8_t *t, int64_t n, int64_t w, uint8_t *b)
{
	const int64_t at = 16 * w, left = n - at;
	if (left >= 16) { const FqWord16 v = *(const FqWord16 *)__builtin_assume_aligned(t + at, 16); memcpy(b, &v, 16); return 16; }
	for (int k = 0; k < (int)left; ++k) b[k] = t[at + k];
	return (int)left;
}
// word w walked from state s (1: header): on_start(i) at a '>' that opens a header, on_end(i) at the '\n' that closes one, on_base(i, byte)
template <class B, class E, class S> ARX_DEVI void fa_walk(const uint8_t *t, int64_t n, int64_t w, int s, B on_base, E on_end, S on_start)
{
	uint8_t b[16];
	const int m = fa_load(t, n, w, b);
	for (int i = 0; i < m; ++i) {
		const uint8_t ch = b[i];
		if (s) { if (ch == '\n') { s = 0; on_end(i); } continue; }
		if (ch == '>') { s = 1; on_start(i); continue; }
		if (ch == '\n' || ch == '\r' || ch == ' ' || ch == '\t') continue;
		on_base(i, ch);
	}
}
// the state, and what stands in front of a base, at the start of word w, from the running maxima and the carry
ARX_DEVI int fa_state_in(const int32_t *hm, int64_t w, int32_t carry) { const int32_t v = w ? hm[w - 1] : 0; return v ? v & 1 : carry; }
ARX_DEVI int32_t fa_prev_in(const int32_t *ev, int64_t w, int32_t carry) { const int32_t v = w ? ev[w - 1] : 0; return v ? v & 0x3ff : carry; }

struct FaMapF {
	const uint8_t *t; int64_t n; int32_t *hm;
	ARX_DEVI void operator()(int64_t w) const
	{
		uint8_t b[16];
		const int m = fa_load(t, n, w, b);
		int32_t v = 0;
		for (int i = 0; i < m; ++i)
			if (b[i] == '>' || b[i] == '\n') v = (int32_t)((w + 1) << 1) | (b[i] == '>');
		hm[w] = v;
	}
};
struct FaCountF {
	const uint8_t *t; int64_t n; const int32_t *hm; int32_t in_hdr; int32_t *ev; int64_t *ca;
	ARX_DEVI void operator()(int64_t w) const
	{
		int64_t nb = 0, na = 0;
		int32_t last = 0;
		fa_walk(t, n, w, fa_state_in(hm, w, in_hdr),
		        [&](int, uint8_t ch) { ++nb; na += fa_code(ch) >= 4; last = FA_EV_BASE | ch; }, [&](int) { last = FA_EV_START; }, [&](int) {});
		ev[w] = last ? (int32_t)((w + 1) << 10) | last : 0;
		ca[w] = nb | na << 32;
	}
};
struct FaHoleF {
	const uint8_t *t; int64_t n; const int32_t *hm, *ev; int32_t in_hdr, lasts; int64_t *cb;
	ARX_DEVI void operator()(int64_t w) const
	{
		int64_t ne = 0, nh = 0;
		int32_t prev = fa_prev_in(ev, w, lasts);
		fa_walk(t, n, w, fa_state_in(hm, w, in_hdr),
		        [&](int, uint8_t ch) { nh += fa_code(ch) >= 4 && prev != (FA_EV_BASE | ch); prev = FA_EV_BASE | ch; }, [&](int) { ++ne; prev = FA_EV_START; }, [&](int) {});
		cb[w] = ne | nh << 32;
	}
};
// the carry of the counts in front of a window
struct FaBase { int64_t file_off, l_pac, n_amb, n_holes, n_contigs; int32_t in_hdr, lasts, n_codes; };
struct FaEmitF {
	const uint8_t *t; int64_t n; const int32_t *hm, *ev; const int64_t *oa, *ob; FaBase c; uint8_t *codes; FaContig *contigs; FaHole *holes; int32_t *meta;
	ARX_DEVI void operator()(int64_t w) const
	{
		int64_t nb = oa[w] & 0xffffffff, na = oa[w] >> 32, ne = ob[w] & 0xffffffff, nh = ob[w] >> 32;
		int32_t prev = fa_prev_in(ev, w, c.lasts);
		uint64_t x = 0;
		bool have_x = false;
		const int64_t at = c.file_off + 16 * w;
		fa_walk(t, n, w, fa_state_in(hm, w, c.in_hdr),
		        [&](int, uint8_t ch) {
			        if (c.n_contigs + ne == 0) meta[0] = 1; // a base before the first contig
			        int code = fa_code(ch);
			        if (code >= 4) {
				        const int64_t k = c.n_amb + na;
				        if (prev != (FA_EV_BASE | ch)) { holes[c.n_holes + nh] = FaHole{c.l_pac + nb, k, ch, 0}; ++nh; }
				        x = have_x ? fa_rand_step(x) : fa_rand_at((uint64_t)k + 1);
				        have_x = true;
				        code = (int)(x >> 17) & 3;
				        ++na;
			        }
			        codes[c.n_codes + nb] = (uint8_t)code;
			        ++nb;
			        prev = FA_EV_BASE | ch;
		        },
		        [&](int i) {
			        FaContig &r = contigs[c.n_contigs + ne];
			        r.hdr_e = at + i; r.off = c.l_pac + nb; r.hole0 = c.n_holes + nh;
			        ++ne;
			        prev = FA_EV_START;
		        },
		        [&](int i) { contigs[c.n_contigs + ne].hdr_b = at + i + 1; });
	}
};
struct FaCopyF { // the carried codes between their place and the window's code list
	const uint8_t *src; uint8_t *dst;
	ARX_DEVI void operator()(int64_t i) const { dst[i] = src[i]; }
};
struct FaZeroF {
	int32_t *p;
	ARX_DEVI void operator()(int64_t i) const { p[i] = 0; }
};
// item: 16 bytes of .pac from 64 codes; n: the codes there are (a multiple of 64 but in the call's last launch)
struct FaPackF {
	const uint8_t *codes; int64_t n; uint8_t *pac; uint64_t *ca, *cb;
	ARX_DEVI static uint32_t four(uint32_t w) { return (w & 3) << 6 | (w >> 8 & 3) << 4 | (w >> 16 & 3) << 2 | (w >> 24 & 3); }
	ARX_DEVI void operator()(int64_t j) const
	{
		const int64_t at = 64 * j, left = n - at;
		uint32_t c1 = 0, c2 = 0, c3 = 0;
		if (left >= 64) {
			FqWord16 o;
			for (int q = 0; q < 4; ++q) {
				const FqWord16 v = *(const FqWord16 *)__builtin_assume_aligned(codes + at + 16 * q, 16);
				o.w[q] = four(v.w[0]) | four(v.w[1]) << 8 | four(v.w[2]) << 16 | four(v.w[3]) << 24;
				for (int k = 0; k < 4; ++k) {
					const uint32_t l = v.w[k] & 0x01010101u, h = v.w[k] >> 1 & 0x01010101u, both = (uint32_t)__builtin_popcount(l & h);
					c3 += both; c1 += (uint32_t)__builtin_popcount(l) - both; c2 += (uint32_t)__builtin_popcount(h) - both;
				}
			}
			*(FqWord16 *)__builtin_assume_aligned(pac + 16 * j, 16) = o;
		} else {
			for (int64_t b = 0; 4 * b < left; ++b) {
				uint8_t acc = 0;
				for (int k = 0; k < 4 && 4 * b + k < left; ++k) {
					const uint8_t code = codes[at + 4 * b + k];
					acc |= (uint8_t)(code << ((3 - k) << 1));
					c1 += code == 1; c2 += code == 2; c3 += code == 3;
				}
				pac[16 * j + b] = acc;
			}
		}
		const uint32_t c0 = (uint32_t)(left >= 64 ? 64 : left) - c1 - c2 - c3;
		ca[j] = (uint64_t)c0 | (uint64_t)c1 << 32; cb[j] = (uint64_t)c2 | (uint64_t)c3 << 32;
	}
};
// the lengths, when the input has ended: a contig reaches to the next one's first base, a hole to the next one's first ambiguous base
struct FaContigFinF {
	FaContig *r; int64_t n, l_pac, n_holes; int32_t *meta;
	ARX_DEVI void operator()(int64_t c) const
	{
		const int64_t len = (c + 1 < n ? r[c + 1].off : l_pac) - r[c].off;
		if (len > 0x7fffffff) meta[1] = 1;
		r[c].len = (int32_t)len;
		r[c].n_holes = (int32_t)((c + 1 < n ? r[c + 1].hole0 : n_holes) - r[c].hole0);
	}
};
struct FaHoleFinF {
	FaHole *h; int64_t n, n_amb;
	ARX_DEVI void operator()(int64_t k) const { h[k].len = (int32_t)((k + 1 < n ? h[k + 1].aord : n_amb) - h[k].aord); }
};

// what a call carries from window to window, and what it has when the input has ended
struct FaState {
	int32_t in_hdr = 0, lasts = 0, n_codes = 0; // lasts: 0 before the first contig
	int64_t file_off = 0, l_pac = 0, n_amb = 0, n_holes = 0, n_contigs = 0, windows = 0;
	uint64_t cnt[4] = {0, 0, 0, 0};
	bool bad_start = false, contig_too_long = false;
	std::string open_hdr;              // the text so far of a header that a window cut
	std::vector<std::string> headers;  // the text of every closed header, '\r's and all
	int64_t packed() const { return l_pac - n_codes; }
	int64_t pac_bytes() const { return (l_pac + 3) / 4; }
};

template <class Drv> void fa_pack_launch(Drv &drv, FaState &S, const uint8_t *codes, int64_t n)
{
	const int64_t groups = (n + 63) / 64, at = S.packed() / 4;
	uint8_t *pac = (uint8_t *)drv.keep(FA_K_PAC, at + (n + 3) / 4, at);
	uint64_t *pa = (uint64_t *)drv.work(FA_W_PCA, 8 * groups), *pb = (uint64_t *)drv.work(FA_W_PCB, 8 * groups);
	drv.items("fa_pack", groups, FaPackF{codes, n, pac + at, pa, pb});
	const uint64_t a = drv.sum64(pa, groups), b = drv.sum64(pb, groups);
	S.cnt[0] += a & 0xffffffff; S.cnt[1] += a >> 32; S.cnt[2] += b & 0xffffffff; S.cnt[3] += b >> 32;
}

// one window: t[0, n) in the driver's memory, 16-byte aligned, 0 < n <= FA_MAX_WINDOW
template <class Drv> int fa_window(Drv &drv, FaState &S, const uint8_t *t, int64_t n)
{
	const int64_t nw = (n + 15) / 16;
	++S.windows;
	int32_t *hm = (int32_t *)drv.work(FA_W_HMAP, 4 * nw), *ev = (int32_t *)drv.work(FA_W_EV, 4 * nw);
	int64_t *ca = (int64_t *)drv.work(FA_W_CNTA, 8 * nw), *oa = (int64_t *)drv.work(FA_W_OFFA, 8 * (nw + 1));
	int64_t *cb = (int64_t *)drv.work(FA_W_CNTB, 8 * nw), *ob = (int64_t *)drv.work(FA_W_OFFB, 8 * (nw + 1));
	int32_t *meta = (int32_t *)drv.work(FA_W_META, 8);
	drv.items("fa_zero", 2, FaZeroF{meta});
	drv.items("fa_maps", nw, FaMapF{t, n, hm});
	drv.scanmax32(hm, nw);
	drv.items("fa_count", nw, FaCountF{t, n, hm, S.in_hdr, ev, ca});
	drv.scanmax32(ev, nw);
	drv.scan(ca, oa, nw);
	drv.items("fa_holes", nw, FaHoleF{t, n, hm, ev, S.in_hdr, S.lasts, cb});
	drv.scan(cb, ob, nw);
	const int64_t ta = drv.get(oa + nw), tb = drv.get(ob + nw);
	const int64_t nb = ta & 0xffffffff, na = ta >> 32, ne = tb & 0xffffffff, nh = tb >> 32;
	const int32_t hm_last = drv.get32(hm + nw - 1), ev_last = drv.get32(ev + nw - 1);
	const int32_t out_hdr = hm_last ? hm_last & 1 : S.in_hdr;
	if (S.n_contigs + ne > 0x7fffffff || S.n_holes + nh > 0x7fffffff) return FA_E_COUNT;
	FaContig *contigs = (FaContig *)drv.keep(FA_K_CONTIGS, (int64_t)sizeof(FaContig) * (S.n_contigs + ne + 1), (int64_t)sizeof(FaContig) * (S.n_contigs + S.in_hdr));
	FaHole *holes = (FaHole *)drv.keep(FA_K_HOLES, (int64_t)sizeof(FaHole) * (S.n_holes + nh), (int64_t)sizeof(FaHole) * S.n_holes);
	uint8_t *carry = (uint8_t *)drv.keep(FA_K_CARRY, 64, 64);
	const int64_t total = S.n_codes + nb, full = total / 64 * 64;
	uint8_t *codes = (uint8_t *)drv.work(FA_W_CODES, (total + 15) / 16 * 16);
	drv.items("fa_carry_in", S.n_codes, FaCopyF{carry, codes});
	drv.items("fa_emit", nw, FaEmitF{t, n, hm, ev, oa, ob, FaBase{S.file_off, S.l_pac, S.n_amb, S.n_holes, S.n_contigs, S.in_hdr, S.lasts, S.n_codes}, codes, contigs, holes, meta});
	if (full) fa_pack_launch(drv, S, codes, full);
	drv.items("fa_carry_out", total - full, FaCopyF{codes + full, carry});
	if (drv.get32(meta)) S.bad_start = true;
	// the headers: what this window holds of their text
	const int64_t rows = ne + out_hdr;
	if (rows) {
		std::vector<FaContig> r((size_t)rows);
		drv.fetch(r.data(), contigs + S.n_contigs, (size_t)rows * sizeof(FaContig));
		auto piece = [&](int64_t a, int64_t b) { // the file's bytes [a, b), as far as they lie in this window
			if (a < S.file_off) a = S.file_off;
			std::string s((size_t)(b > a ? b - a : 0), '\0');
			if (b > a) drv.fetch(&s[0], t + (a - S.file_off), (size_t)(b - a));
			return s;
		};
		for (int64_t k = 0; k < ne; ++k) {
			S.headers.push_back(S.open_hdr + piece(r[(size_t)k].hdr_b, r[(size_t)k].hdr_e)); // (open_hdr is empty but for a header cut before this window)
			S.open_hdr.clear();
		}
		if (out_hdr) S.open_hdr += piece(ne == 0 && S.in_hdr ? S.file_off : r[(size_t)ne].hdr_b, S.file_off + n);
	}
	S.in_hdr = out_hdr;
	if (ev_last) S.lasts = ev_last & 0x3ff;
	S.file_off += n; S.l_pac += nb; S.n_amb += na; S.n_holes += nh; S.n_contigs += ne;
	S.n_codes = (int32_t)(total - full);
	return FA_OK;
}

// the input has ended: the last codes, the lengths.  contigs / holes: the rows, read home
template <class Drv> void fa_finish(Drv &drv, FaState &S, std::vector<FaContig> &contigs, std::vector<FaHole> &holes)
{
	if (S.n_codes) {
		uint8_t *carry = (uint8_t *)drv.keep(FA_K_CARRY, 64, 64);
		fa_pack_launch(drv, S, carry, S.n_codes); // behind what is packed: l_pac - n_codes bases
		S.n_codes = 0;
	}
	int32_t *meta = (int32_t *)drv.work(FA_W_META, 8);
	drv.items("fa_zero", 2, FaZeroF{meta});
	contigs.assign((size_t)S.n_contigs, FaContig{});
	holes.assign((size_t)S.n_holes, FaHole{});
	if (S.n_contigs) {
		FaContig *r = (FaContig *)drv.keep(FA_K_CONTIGS, (int64_t)sizeof(FaContig) * (S.n_contigs + 1), (int64_t)sizeof(FaContig) * (S.n_contigs + S.in_hdr));
		drv.items("fa_contig_fin", S.n_contigs, FaContigFinF{r, S.n_contigs, S.l_pac, S.n_holes, meta});
		drv.fetch(contigs.data(), r, contigs.size() * sizeof(FaContig));
	}
	if (S.n_holes) {
		FaHole *h = (FaHole *)drv.keep(FA_K_HOLES, (int64_t)sizeof(FaHole) * S.n_holes, (int64_t)sizeof(FaHole) * S.n_holes);
		drv.items("fa_hole_fin", S.n_holes, FaHoleFinF{h, S.n_holes, S.n_amb});
		drv.fetch(holes.data(), h, holes.size() * sizeof(FaHole));
	}
	int32_t m[2] = {0, 0};
	drv.fetch(m, meta, 8);
	if (m[1]) S.contig_too_long = true;
}

} // namespace arx

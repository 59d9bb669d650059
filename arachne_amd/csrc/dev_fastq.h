// dev_fastq.h -- the per-byte work of the device FASTQ feeder (device_feeder.h) as functors over raw file text in device memory:
// line index, record recognition, header fields, base codes, barcode runs.  Rule for rule what feeder.h does on the host
// (LineSource::next, Feeder::read_one, parse_header, append_read); tests/test_device_feeder.py holds both to the restatement.
//
// A "window" is the text of one file the parse looks at: the bytes carried over from the last parse followed by new chunks.  All
// positions are byte offsets into the window of their file.  Only lines that end in '\n' exist; line j of a file is
// [j ? nl[j - 1] + 1 : 0, nl[j]).  Lines 0 .. L-1 (L = the smaller of the two files' line counts) are walked in lockstep.
//
// Launch order (device_feeder.h: DeviceFeeder::parse_window), every functor through launch_wide, scans through exclusive_scan:
//   KNlCount            newlines per 16-byte word of both windows            -> scan -> the two line counts
//   KNlFill             positions of the newlines
//   KLineMaps           which line pairs may start a record; composed state map of each block of FQ_LINE_BLOCK line pairs
//   KLineStates         (one item) state at the start of every block; where the carry starts if no record is cut off
//   KRecCount           records that start in each block                      -> scan -> number of complete records
//   KRecFill            header line of every record
//   KRecParse           header fields and lengths of every record
//   KRunFlag            does record r open a barcode run                      -> scan over lens | name | rg | run | run barcode lengths
//   KTotals             (one item) the five totals of that scan
//   KFillReads, KFillRecords   bases, quals, names, rgs, valid, run list into one output blob
#pragma once
#include <stdint.h>

namespace arx {

constexpr int FQ_LINE_BLOCK = 256; // line pairs per item of the state scan

// record recognition: state 0 = searching for a header, 1..3 = that many lines of a record still to pass unseen.  A line pair maps
// every state to the next one; the map is 2 bits per input state (8 bits), and maps compose associatively.
ARX_HDI uint32_t fq_line_map(bool header) { return header ? 0x93u : 0x90u; }          // 0 -> 3 or 0, 1 -> 0, 2 -> 1, 3 -> 2
ARX_HDI uint32_t fq_map_apply(uint32_t m, uint32_t s) { return (m >> (2 * s)) & 3u; }
ARX_HDI uint32_t fq_map_compose(uint32_t first, uint32_t then)
{
	uint32_t r = 0;
	for (uint32_t s = 0; s < 4; ++s) r |= fq_map_apply(then, fq_map_apply(first, s)) << (2 * s);
	return r;
}

ARX_HDI bool fq_is_space(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }
ARX_HDI uint8_t fq_nt4(uint8_t c) // nst_nt4_table (bntseq.c:47)
{
	const uint8_t l = c | 0x20;
	return l == 'a' ? 0 : l == 'c' ? 1 : l == 'g' ? 2 : l == 't' ? 3 : 4;
}
// bit 8k+7 set for every byte k of w that equals '\n' (exact: no carry between bytes)
ARX_HDI uint32_t fq_nl_mask(uint32_t w)
{
	const uint32_t x = w ^ 0x0A0A0A0Au;
	return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
ARX_HDI int fq_popc(uint32_t x) { x = x - ((x >> 1) & 0x55555555u); x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u); return (int)((((x + (x >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24); }

struct alignas(16) FqWord16 { uint32_t w[4]; };

// the two windows: text (16-byte aligned, readable up to the next multiple of 16 past n) and length
struct FqWin {
	const uint8_t *t1, *t2;
	int32_t n1, n2;
	int32_t nw1, nw2; // 16-byte words: (n + 15) / 16
};

// masks of the newlines of word i of a window (bytes at or past n do not count)
ARX_DEVI void fq_word_masks(const uint8_t *t, int32_t n, int i, uint32_t m[4])
{
	const FqWord16 v = *(const FqWord16 *)(t + (size_t)i * 16);
	for (int k = 0; k < 4; ++k) {
		uint32_t x = fq_nl_mask(v.w[k]);
		const int32_t left = n - (i * 16 + k * 4); // bytes of this word inside the window
		if (left < 4) x = left <= 0 ? 0u : x & (0x80808080u >> (8 * (4 - left)));
		m[k] = x;
	}
}

struct KNlCount { // item: one 16-byte word of window 1 (i < nw1) or of window 2
	FqWin w;
	int32_t *cnt; // nw1 + nw2
	ARX_DEV void operator()(int i, int) const
	{
		uint32_t m[4];
		if (i < w.nw1) fq_word_masks(w.t1, w.n1, i, m); else fq_word_masks(w.t2, w.n2, i - w.nw1, m);
		cnt[i] = fq_popc(m[0]) + fq_popc(m[1]) + fq_popc(m[2]) + fq_popc(m[3]);
	}
};

struct KNlFill { // nl[off[i] ..]: positions of the word's newlines; window 2's follow window 1's in nl, as in the scan
	FqWin w;
	const int32_t *off;
	int32_t *nl;
	ARX_DEV void operator()(int i, int) const
	{
		uint32_t m[4];
		const int wi = i < w.nw1 ? i : i - w.nw1;
		if (i < w.nw1) fq_word_masks(w.t1, w.n1, wi, m); else fq_word_masks(w.t2, w.n2, wi, m);
		int32_t *o = nl + off[i];
		for (int k = 0; k < 4; ++k)
			for (int b = 0; b < 4; ++b)
				if (m[k] >> (8 * b + 7) & 1u) *o++ = wi * 16 + k * 4 + b;
	}
};

// the line index of both windows, L line pairs
struct FqLines {
	const uint8_t *t1, *t2;
	const int32_t *nl1, *nl2;
	int32_t L;
	ARX_DEVI int32_t start1(int j) const { return j ? nl1[j - 1] + 1 : 0; }
	ARX_DEVI int32_t start2(int j) const { return j ? nl2[j - 1] + 1 : 0; }
	// Feeder::read_one: a line pair starts a record if the R1 line is non-empty and starts with '@'
	ARX_DEVI bool header(int j) const { const int32_t s = start1(j); return nl1[j] > s && t1[s] == '@'; }
};

struct KLineMaps { // item: one block of line pairs; the only pass that looks at the text: hdr[j] keeps "line pair j may start a record"
	FqLines ln;
	uint8_t *bmap, *hdr;
	ARX_DEV void operator()(int i, int) const
	{
		const int j0 = i * FQ_LINE_BLOCK, j1 = j0 + FQ_LINE_BLOCK < ln.L ? j0 + FQ_LINE_BLOCK : ln.L;
		uint32_t m = 0xE4u; // identity
		for (int j = j0; j < j1; ++j) { const bool h = ln.header(j); hdr[j] = h; m = fq_map_compose(m, fq_line_map(h)); }
		bmap[i] = (uint8_t)m;
	}
};

// meta (int32 words the host reads after the parse): [0] carry start in window 1, [1] in window 2, [2] line the carry starts at,
// [3..7] totals of the output scan: bases, name bytes, rg bytes, runs, run barcode bytes
struct KLineStates { // one item: the scan across blocks, seeded with the state the bytes before ended in
	FqLines ln;
	const uint8_t *bmap;
	uint8_t *bstate;
	int32_t n_blocks, seed;
	int32_t *meta;
	ARX_DEV void operator()(int, int) const
	{
		uint32_t s = (uint32_t)seed;
		for (int b = 0; b < n_blocks; ++b) { bstate[b] = (uint8_t)s; s = fq_map_apply(bmap[b], s); }
		// unless KRecCount finds a record that the windows cut off, everything up to line L is consumed
		meta[0] = ln.start1(ln.L); meta[1] = ln.start2(ln.L); meta[2] = ln.L;
	}
};

struct KRecCount { // item: one block; counts the records that start in it and are complete in both windows (four line pairs)
	FqLines ln;
	const uint8_t *bstate, *hdr;
	int32_t *cnt, *meta;
	ARX_DEV void operator()(int i, int) const
	{
		const int j0 = i * FQ_LINE_BLOCK, j1 = j0 + FQ_LINE_BLOCK < ln.L ? j0 + FQ_LINE_BLOCK : ln.L;
		uint32_t s = bstate[i];
		int c = 0;
		for (int j = j0; j < j1; ++j) {
			const bool h = hdr[j];
			if (s == 0 && h) {
				if (j + 3 < ln.L) ++c;
				else { meta[0] = ln.start1(j); meta[1] = ln.start2(j); meta[2] = j; } // at most one: the last record, carried whole
			}
			s = fq_map_apply(fq_line_map(h), s);
		}
		cnt[i] = c;
	}
};

struct KRecFill {
	FqLines ln;
	const uint8_t *bstate, *hdr;
	const int32_t *off;
	int32_t *rec_line;
	ARX_DEV void operator()(int i, int) const
	{
		const int j0 = i * FQ_LINE_BLOCK, j1 = j0 + FQ_LINE_BLOCK < ln.L ? j0 + FQ_LINE_BLOCK : ln.L;
		uint32_t s = bstate[i];
		int32_t *o = rec_line + off[i];
		for (int j = j0; j < j1; ++j) {
			const bool h = hdr[j];
			if (s == 0 && h && j + 3 < ln.L) *o++ = j;
			s = fq_map_apply(fq_line_map(h), s);
		}
	}
};

// what KRecParse leaves per record: positions in window 1 of the three header fields (their lengths go into the scan input)
struct FqRecTmp { int32_t name_pos, rg_pos, bc_pos, bc_len; };

// scan input of n records, 6n int32: [0, 2n) read lengths | [2n, 3n) name lengths | [3n, 4n) rg lengths | [4n, 5n) opens a run |
// [5n, 6n) barcode length where it opens a run
struct KRecParse { // item: one record; parse_header (feeder.h) on the R1 header, the two sequence lengths
	FqLines ln;
	const int32_t *rec_line;
	int32_t n;
	FqRecTmp *tmp;
	int32_t *sc;
	uint8_t *valid;
	ARX_DEV void operator()(int r, int) const
	{
		const int j = rec_line[r];
		const uint8_t *t = ln.t1;
		const int32_t b = ln.start1(j) + 1, e = ln.nl1[j]; // the header without its '@' and '\n'
		sc[2 * r] = ln.nl1[j + 1] - ln.start1(j + 1);
		sc[2 * r + 1] = ln.nl2[j + 1] - ln.start2(j + 1);
		// first and last whitespace-separated token
		int32_t p = b;
		while (p < e && fq_is_space(t[p])) ++p;
		const int32_t f0 = p;
		while (p < e && !fq_is_space(t[p])) ++p;
		const int32_t f0e = p;
		int n_fields = f0e > f0;
		int32_t lb = f0, le = f0e;
		while (p < e) {
			while (p < e && fq_is_space(t[p])) ++p;
			if (p >= e) break;
			lb = p;
			while (p < e && !fq_is_space(t[p])) ++p;
			le = p; ++n_fields;
		}
		FqRecTmp o;
		o.rg_pos = lb; sc[3 * n + r] = n_fields >= 2 ? le - lb : 0;
		// leftmost BX:Z:(\S+)\s -- the line's own '\n' closes a value at the end of the line
		bool have_bc = false;
		o.bc_pos = b; o.bc_len = 0;
		for (p = b; p + 5 <= e; ++p) {
			if (t[p] != 'B' || t[p + 1] != 'X' || t[p + 2] != ':' || t[p + 3] != 'Z' || t[p + 4] != ':') continue;
			const int32_t v = p + 5;
			if (v >= e || fq_is_space(t[v])) continue;
			int32_t w = v;
			while (w < e && !fq_is_space(t[w])) ++w;
			o.bc_pos = v; o.bc_len = w - v; have_bc = true;
			break;
		}
		// ReadInfo: the first token minus its last two bytes, and only with a barcode
		o.name_pos = f0; sc[2 * n + r] = have_bc && f0e - f0 >= 2 ? f0e - f0 - 2 : 0;
		uint8_t ok = 0;
		if (have_bc)
			for (p = b; p + 6 <= e; ++p) { // VX:i:[01]\s
				if (t[p] != 'V' || t[p + 1] != 'X' || t[p + 2] != ':' || t[p + 3] != 'i' || t[p + 4] != ':') continue;
				const uint8_t d = t[p + 5];
				if ((d == '0' || d == '1') && (p + 6 == e || fq_is_space(t[p + 6]))) { ok = d == '1'; break; }
			}
		valid[r] = ok;
		tmp[r] = o;
	}
};

struct KRunFlag { // record r opens a run iff its barcode (bytes and length) differs from record r-1's; record 0 is settled on the host
	const uint8_t *t1;
	const FqRecTmp *tmp;
	int32_t n;
	int32_t *sc;
	ARX_DEV void operator()(int r, int) const
	{
		const FqRecTmp a = tmp[r];
		bool open = true;
		if (r > 0) {
			const FqRecTmp q = tmp[r - 1];
			open = q.bc_len != a.bc_len;
			for (int k = 0; !open && k < a.bc_len; ++k) open = t1[q.bc_pos + k] != t1[a.bc_pos + k];
		}
		sc[4 * n + r] = open; sc[5 * n + r] = open ? a.bc_len : 0;
	}
};

struct KTotals {
	const int32_t *so; // the scan of sc: 6n + 1
	int32_t n;
	int32_t *meta;
	ARX_DEV void operator()(int, int) const
	{
		meta[3] = so[2 * n];
		for (int k = 1; k < 5; ++k) meta[3 + k] = so[(2 + k) * n] - so[(1 + k) * n];
	}
};

// the output blob of one parse (device pointers into it; the host copies it home in one piece)
struct FqOut {
	int32_t *lens;      // 2n
	int32_t *rec_line;  // n   header line of the record (the host derives the lines skipped before it)
	int32_t *name_len, *rg_len; // n each
	int32_t *run_first; // R   first record of the run
	int32_t *run_bc_off;// R + 1
	uint8_t *bases, *quals; // B each
	uint8_t *names, *rgs, *valid, *run_bc;
};

struct KFillReads { // item: one read (2r: R1, 2r + 1: R2): base codes, and the quality line cut or padded with '!' to the sequence (append_read)
	FqLines ln;
	const int32_t *rec_line, *so;
	FqOut o;
	ARX_DEV void operator()(int k, int) const
	{
		const int j = rec_line[k >> 1];
		const bool two = k & 1;
		const uint8_t *t = two ? ln.t2 : ln.t1;
		const int32_t s = two ? ln.start2(j + 1) : ln.start1(j + 1), len = so[k + 1] - so[k];
		const int32_t q = two ? ln.start2(j + 3) : ln.start1(j + 3), qlen = (two ? ln.nl2[j + 3] : ln.nl1[j + 3]) - q;
		uint8_t *ob = o.bases + so[k], *oq = o.quals + so[k];
		for (int32_t x = 0; x < len; ++x) { ob[x] = fq_nt4(t[s + x]); oq[x] = x < qlen ? t[q + x] : (uint8_t)'!'; }
		o.lens[k] = len;
	}
};

struct KFillRecords { // item: one record: name, rg, valid, header line, and its run's entry if it opens one
	const uint8_t *t1;
	const FqRecTmp *tmp;
	const int32_t *sc, *so, *rec_line;
	const uint8_t *valid;
	int32_t n;
	FqOut o;
	ARX_DEV void operator()(int r, int) const
	{
		const FqRecTmp a = tmp[r];
		const int32_t nl_ = sc[2 * n + r], gl = sc[3 * n + r];
		o.rec_line[r] = rec_line[r]; o.valid[r] = valid[r];
		uint8_t *on = o.names + (so[2 * n + r] - so[2 * n]), *og = o.rgs + (so[3 * n + r] - so[3 * n]);
		for (int32_t x = 0; x < nl_; ++x) on[x] = t1[a.name_pos + x];
		for (int32_t x = 0; x < gl; ++x) og[x] = t1[a.rg_pos + x];
		o.name_len[r] = nl_; o.rg_len[r] = gl;
		if (sc[4 * n + r]) {
			const int32_t k = so[4 * n + r] - so[4 * n], at = so[5 * n + r] - so[5 * n];
			o.run_first[k] = r; o.run_bc_off[k] = at;
			for (int32_t x = 0; x < a.bc_len; ++x) o.run_bc[at + x] = t1[a.bc_pos + x];
		}
		if (r == n - 1) o.run_bc_off[so[5 * n] - so[4 * n]] = so[6 * n] - so[5 * n];
	}
};

} // namespace arx

// dev_fqstd.h -- the step in front of the FASTQ sort: the headers of a haplotagging, stLFR or TELLseq file pair rewritten to the form the feeder
// and the sort read, `@<id>/1\tBX:Z:<barcode>\tVX:i:<0|1>` (the intended behaviour of the reference's src/preprocess/standardize.go, which does
// not compile; include/arachne_amd.h states the contract and lists the repairs).  As dev_fqsort.h it is launches over an explicit item index,
// shared by the kernels' driver (hip_fqstd.h) and the host program (tests/fqstdsim/fastq_std_sim.cpp) through the same `drv`:
//     drv.items / scan / scan32 / max64 / get / get32 / fetch / work      as dev_fqsort.h has them (no sort and no table are needed)
//     drv.phase(k)                                                        what the host does next (FQS_P_*): a clock's business, nothing else
// the source  src.fill(f, dst, want) -> the bytes put at dst, fewer than `want` only at the file's end; src.ended(f): nothing is left of file f
// the sink    take / give, as fs_gather's
//
// The stream.  The call never holds a file: per file two window buffers of window_bytes.  A window is what the parse before did not consume (the
// carry, moved to the other buffer's front by FsWindowF, as the feeder moves it) followed by new bytes up to window_bytes.  The feeder's own
// functors make the line index and find the records (KNlCount ... KRecFill: what a record is stays the feeder's business); a parse consumes
// the line pairs both windows hold up to the last record that is whole in both, so every window starts in the search state.  A window of which
// not one line pair can be consumed is FS_E_TOO_LARGE.  The end-of-input rule is the sort's: a file that has ended and has no line left ends
// the input.
//
// Per window (fqs_convert): FqsFieldsF, one item per record, finds id, barcode and validity for the one format of the call and the record's two
// output sizes; their prefix sums say where every record goes; slabs are cut as the sort cuts them (records whose bytes fit slab_bytes in
// both files, one at least); FqsComposeF writes a slab, FS_GATHER_LANES lanes per (record, file): the synthesized header resolved per output
// byte, lines 2-4 copied by bs_copy at the destination's alignment.  No byte is written twice, there are no atomics, nothing depends on the
// order of the items.  Detection (fqs_detect) is a pass of its own over the head of the input: FqsMatchF, one item per record, runs the four
// matchers in one pass over the header and leaves a class byte; the first of records 0..199 with a class decides.
#pragma once
#include <vector>
#include "dev_fqsort.h"

namespace arx {

enum { FQS_AUTO = 0, FQS_HAPLOTAGGING = 1, FQS_STLFR = 2, FQS_TELLSEQ = 3, FQS_STANDARD = 4, FQS_UNKNOWN = 5 }; // ARX_FQSTD_* (include/arachne_amd.h)
constexpr int64_t FQS_DETECT_RECORDS = 200; // findFastqFormat looks at so many records
constexpr int FQS_FIXED = 17;               // '@' "/1\tBX:Z:" "\tVX:i:" digit '\n'
enum { FQS_P_FILL = 0, FQS_P_PARSE, FQS_P_COMPOSE };
// the sort's work slots that this step has no other use for, under its own names
enum { FQS_W_WIN1A = FS_W_WIN1, FQS_W_WIN2A = FS_W_WIN2, FQS_W_WIN1B = FS_W_STAGE1, FQS_W_WIN2B = FS_W_STAGE2, FQS_W_CLASS = FS_W_VALID, FQS_W_FLD = FS_W_TMP,
       FQS_W_S1 = FS_W_KEYS0, FQS_W_S2 = FS_W_KEYS1, FQS_W_O1 = FS_W_OUT1, FQS_W_O2 = FS_W_OUT2, FQS_W_CNT = FS_W_VALS0, FQS_W_CNTO = FS_W_VALS1, FQS_W_BCL = FS_W_KOFF };

// ---- the matchers.  H = t[b, E): the R1 header without its '@', its own '\n' (t[E - 1]) standing as closing white space.  Each is "does the
// pattern match AT p", decided by one forward scan; no byte at or behind E is read
ARX_DEVI bool fqs_digit(uint8_t c) { return c >= '0' && c <= '9'; }
ARX_DEVI bool fqs_tag(const uint8_t *t, int32_t p, int32_t E, uint8_t a, uint8_t b, uint8_t c)
{
	return p + 5 <= E && t[p] == a && t[p + 1] == b && t[p + 2] == ':' && t[p + 3] == c && t[p + 4] == ':';
}
// BX:Z:(\S+)\s -> the value
ARX_DEVI bool fqs_bx_at(const uint8_t *t, int32_t p, int32_t E, int32_t *pos, int32_t *len)
{
	if (!fqs_tag(t, p, E, 'B', 'X', 'Z')) return false;
	const int32_t v = p + 5;
	int32_t w = v;
	while (w < E && !fq_is_space(t[w])) ++w;
	if (w == v || w >= E) return false;
	*pos = v; *len = w - v;
	return true;
}
// VX:i:([01])\s
ARX_DEVI bool fqs_vx_at(const uint8_t *t, int32_t p, int32_t E)
{
	return fqs_tag(t, p, E, 'V', 'X', 'i') && p + 7 <= E && (t[p + 5] == '0' || t[p + 5] == '1') && fq_is_space(t[p + 6]);
}
// BX:Z:A\d\dC\d\dB\d\dD\d\d\s
ARX_DEVI bool fqs_hap_at(const uint8_t *t, int32_t p, int32_t E)
{
	if (!fqs_tag(t, p, E, 'B', 'X', 'Z') || p + 18 > E) return false;
	const uint8_t *q = t + p + 5;
	return q[0] == 'A' && q[3] == 'C' && q[6] == 'B' && q[9] == 'D' && fqs_digit(q[1]) && fqs_digit(q[2]) && fqs_digit(q[4]) && fqs_digit(q[5]) && fqs_digit(q[7]) &&
	       fqs_digit(q[8]) && fqs_digit(q[10]) && fqs_digit(q[11]) && fq_is_space(q[12]);
}
// #[0-9]+_[0-9]+_[0-9]+(/[12])?\s -> the n_n_n
ARX_DEVI bool fqs_stlfr_at(const uint8_t *t, int32_t p, int32_t E, int32_t *pos, int32_t *len)
{
	if (p >= E || t[p] != '#') return false;
	int32_t q = p + 1;
	for (int g = 0; g < 3; ++g) {
		const int32_t d0 = q;
		while (q < E && fqs_digit(t[q])) ++q;
		if (q == d0) return false;
		if (g < 2) { if (q >= E || t[q] != '_') return false; ++q; }
	}
	const int32_t end = q;
	if (q + 1 < E && t[q] == '/' && (t[q + 1] == '1' || t[q + 1] == '2')) q += 2;
	if (q >= E || !fq_is_space(t[q])) return false;
	*pos = p + 1; *len = end - (p + 1);
	return true;
}
// :[ATCGN]+\s -> the letters
ARX_DEVI bool fqs_tell_at(const uint8_t *t, int32_t p, int32_t E, int32_t *pos, int32_t *len)
{
	if (p >= E || t[p] != ':') return false;
	int32_t q = p + 1;
	while (q < E && (t[q] == 'A' || t[q] == 'T' || t[q] == 'C' || t[q] == 'G' || t[q] == 'N')) ++q;
	if (q == p + 1 || q >= E || !fq_is_space(t[q])) return false;
	*pos = p + 1; *len = q - (p + 1);
	return true;
}

// item: one record.  cls[r]: the first format in the order of trial (standard, haplotagging, stLFR, TELLseq) that its header matches, or 0
struct FqsMatchF {
	FqLines ln; const int32_t *rec_line; uint8_t *cls;
	ARX_DEVI void operator()(int64_t r) const
	{
		const int j = rec_line[r];
		const uint8_t *t = ln.t1;
		const int32_t b = ln.start1(j) + 1, E = ln.nl1[j] + 1;
		bool bx = false, vx = false, hap = false, st = false, te = false;
		int32_t pos, len;
		for (int32_t p = b; p < E; ++p) {
			const uint8_t ch = t[p];
			if (ch == 'B') { bx = bx || fqs_bx_at(t, p, E, &pos, &len); hap = hap || fqs_hap_at(t, p, E); }
			else if (ch == 'V') vx = vx || fqs_vx_at(t, p, E);
			else if (ch == '#') st = st || fqs_stlfr_at(t, p, E, &pos, &len);
			else if (ch == ':') te = te || fqs_tell_at(t, p, E, &pos, &len);
		}
		cls[r] = (uint8_t)(bx && vx ? FQS_STANDARD : hap ? FQS_HAPLOTAGGING : st ? FQS_STLFR : te ? FQS_TELLSEQ : 0);
	}
};

// what FqsFieldsF leaves per record: positions in the windows of id and barcode (window 1) and of lines 2-4 (their own window)
struct FqsRec { int32_t id_pos, id_len, bc_pos, bc_len, body1, blen1, body2, blen2, v, pad; };

// id, barcode and v of H = t[b, E) for `format` (1 .. 3) into o.id_pos .. o.bc_len and o.v, positions counted from t -> the header has a barcode
ARX_DEVI bool fqs_fields(const uint8_t *t, int32_t b, int32_t E, int32_t format, FqsRec &o)
{
	// the id: the first token, one trailing /1 or /2 removed
	int32_t p = b;
	while (p < E && fq_is_space(t[p])) ++p;
	o.id_pos = p;
	while (p < E && !fq_is_space(t[p])) ++p;
	o.id_len = p - o.id_pos;
	if (o.id_len >= 2 && t[p - 2] == '/' && (t[p - 1] == '1' || t[p - 1] == '2')) o.id_len -= 2;
	// the barcode: the leftmost match of the format's pattern
	bool have = false;
	o.bc_pos = b; o.bc_len = 0;
	for (p = b; p < E && !have; ++p)
		have = format == FQS_HAPLOTAGGING ? fqs_bx_at(t, p, E, &o.bc_pos, &o.bc_len) : format == FQS_STLFR ? fqs_stlfr_at(t, p, E, &o.bc_pos, &o.bc_len)
		                                                                                                      : fqs_tell_at(t, p, E, &o.bc_pos, &o.bc_len);
	const uint8_t *c = t + o.bc_pos;
	const int32_t n = o.bc_len;
	bool ok = have;
	if (format == FQS_HAPLOTAGGING) { // no two adjacent '0'
		for (int32_t k = 0; k + 1 < n; ++k) ok = ok && !(c[k] == '0' && c[k + 1] == '0');
	} else if (format == FQS_STLFR) { // not ^0_ | _0_ | _0$
		ok = ok && !(c[0] == '0' && c[1] == '_') && !(c[n - 2] == '_' && c[n - 1] == '0');
		for (int32_t k = 0; k + 2 < n; ++k) ok = ok && !(c[k] == '_' && c[k + 1] == '0' && c[k + 2] == '_');
	} else { // no N
		for (int32_t k = 0; k < n; ++k) ok = ok && c[k] != 'N';
	}
	o.v = ok; o.pad = 0;
	return have;
}

struct FqsFieldsF { // item: one record of a window, for the format of the call
	FqLines ln; const int32_t *rec_line; int32_t format; FqsRec *fld; int64_t *s1, *s2; int64_t *cnt; uint64_t *bcl;
	ARX_DEVI void operator()(int64_t r) const
	{
		const int j = rec_line[r];
		const int32_t b = ln.start1(j) + 1, E = ln.nl1[j] + 1;
		FqsRec o;
		const bool have = fqs_fields(ln.t1, b, E, format, o), ok = o.v != 0;
		o.body1 = ln.start1(j + 1); o.blen1 = ln.nl1[j + 3] + 1 - o.body1;
		o.body2 = ln.start2(j + 1); o.blen2 = ln.nl2[j + 3] + 1 - o.body2;
		fld[r] = o;
		const int64_t h = FQS_FIXED + o.id_len + o.bc_len;
		s1[r] = h + o.blen1; s2[r] = h + o.blen2;
		cnt[r] = (int64_t)have | (int64_t)ok << 32;
		bcl[r] = (uint64_t)o.bc_len;
	}
};

// byte k of the synthesized header of a record for file `two`
ARX_DEVI uint8_t fqs_header_byte(const uint8_t *t1, const FqsRec &r, bool two, int32_t k)
{
	if (k == 0) return '@';
	k -= 1;
	if (k < r.id_len) return t1[r.id_pos + k];
	k -= r.id_len;
	if (k < 8) return k == 0 ? '/' : k == 1 ? (two ? '2' : '1') : k == 2 ? '\t' : k == 3 ? 'B' : k == 4 ? 'X' : k == 6 ? 'Z' : ':';
	k -= 8;
	if (k < r.bc_len) return t1[r.bc_pos + k];
	k -= r.bc_len;
	return k == 0 ? '\t' : k == 1 ? 'V' : k == 2 ? 'X' : k == 4 ? 'i' : k == 6 ? (r.v ? '1' : '0') : k == 7 ? '\n' : ':';
}
struct FqsComposeF { // item: one lane of one file of one record of the slab that starts at record j0 of the window
	const uint8_t *t1, *t2; const FqsRec *fld; const int64_t *o1, *o2; int64_t j0; uint8_t *d1, *d2;
	ARX_DEVI void operator()(int64_t i) const
	{
		const int lane = (int)(i % FS_GATHER_LANES);
		const bool two = (i / FS_GATHER_LANES) & 1;
		const int64_t j = j0 + i / (2 * FS_GATHER_LANES);
		const FqsRec &r = fld[j];
		uint8_t *d = two ? d2 + (o2[j] - o2[j0]) : d1 + (o1[j] - o1[j0]);
		const int32_t h = FQS_FIXED + r.id_len + r.bc_len;
		for (int32_t k = lane; k < h; k += FS_GATHER_LANES) d[k] = fqs_header_byte(t1, r, two, k);
		if (two) bs_copy(d + h, t2 + r.body2, r.blen2, lane, FS_GATHER_LANES);
		else bs_copy(d + h, t1 + r.body1, r.blen1, lane, FS_GATHER_LANES);
	}
};

struct FqsCounts {
	int64_t n_records = 0, skipped = 0, windows = 0, slabs = 0, in1 = 0, in2 = 0, bytes1 = 0, bytes2 = 0, with_bc = 0, valid = 0, max_bc = 0;
	int32_t format = FQS_UNKNOWN; int64_t decided = -1;          // detection: the format found and the record that decided
	std::vector<int64_t> *off1 = nullptr, *off2 = nullptr;       // where the records start in the outputs (n_records + 1), where somebody asks
};
struct FqsWin { FqLines ln; const int32_t *rec_line; int64_t n; }; // the records of one parsed window

// the records of what src delivers, window by window: visit(W) for every window that holds records, c.n_records being the records before it;
// visit -> false ends the stream early.  FS_OK, or FS_E_TOO_LARGE
template <class Drv, class Src, class Visit> int fqs_stream(Drv &drv, Src &src, int64_t window, FqsCounts &c, Visit visit)
{
	const int64_t room = (window + 15) / 16 * 16; // FsWindowF writes whole words, and the line index reads them
	uint8_t *win[2][2] = {{(uint8_t *)drv.work(FQS_W_WIN1A, room), (uint8_t *)drv.work(FQS_W_WIN1B, room)}, {(uint8_t *)drv.work(FQS_W_WIN2A, room), (uint8_t *)drv.work(FQS_W_WIN2B, room)}};
	int64_t have[2] = {0, 0};
	int cur = 0;
	for (;;) {
		drv.phase(FQS_P_FILL);
		for (int f = 0; f < 2; ++f)
			if (!src.ended(f) && have[f] < window) {
				const int64_t k = src.fill(f, win[f][cur] + have[f], window - have[f]);
				have[f] += k; (f ? c.in2 : c.in1) += k;
			}
		drv.phase(FQS_P_PARSE);
		const bool end1 = src.ended(0), end2 = src.ended(1);
		const int32_t nw1 = (int32_t)((have[0] + 15) / 16), nw2 = (int32_t)((have[1] + 15) / 16), nw = nw1 + nw2;
		++c.windows;
		int32_t L1 = 0, L2 = 0;
		const FqWin w{win[0][cur], win[1][cur], (int32_t)have[0], (int32_t)have[1], nw1, nw2};
		const int32_t *nl = nullptr;
		if (nw > 0) {
			int32_t *cnt = (int32_t *)drv.work(FS_W_CNT, 4 * (int64_t)nw), *off = (int32_t *)drv.work(FS_W_OFF, 4 * ((int64_t)nw + 1));
			drv.items("fq_nl_count", nw, fs_wide(KNlCount{w, cnt}));
			const int64_t total = drv.scan32(cnt, off, nw);
			L1 = drv.get32(off + nw1);
			L2 = (int32_t)(total - L1);
			int32_t *nlw = (int32_t *)drv.work(FS_W_NL, 4 * total);
			drv.items("fq_nl_fill", nw, fs_wide(KNlFill{w, off, nlw}));
			nl = nlw;
		}
		const int32_t L = L1 < L2 ? L1 : L2;
		int32_t meta[3] = {0, 0, 0};
		int64_t n = 0;
		if (L > 0) {
			const FqLines ln{w.t1, w.t2, nl, nl + L1, L};
			const int nblk = (L + FQ_LINE_BLOCK - 1) / FQ_LINE_BLOCK;
			uint8_t *bmap = (uint8_t *)drv.work(FS_W_BMAP, nblk), *bstate = (uint8_t *)drv.work(FS_W_BSTATE, nblk), *hdr = (uint8_t *)drv.work(FS_W_HDR, L);
			int32_t *rcnt = (int32_t *)drv.work(FS_W_RCNT, 4 * (int64_t)nblk), *roff = (int32_t *)drv.work(FS_W_ROFF, 4 * ((int64_t)nblk + 1));
			int32_t *dmeta = (int32_t *)drv.work(FS_W_META, 4 * 3);
			drv.items("fq_line_maps", nblk, fs_wide(KLineMaps{ln, bmap, hdr}));
			drv.items("fq_line_states", 1, fs_wide(KLineStates{ln, bmap, bstate, nblk, 0, dmeta}));
			drv.items("fq_rec_count", nblk, fs_wide(KRecCount{ln, bstate, hdr, rcnt, dmeta}));
			n = drv.scan32(rcnt, roff, nblk);
			int32_t *recl = nullptr;
			if (n > 0) {
				recl = (int32_t *)drv.work(FS_W_RECL, 4 * n);
				drv.items("fq_rec_fill", nblk, fs_wide(KRecFill{ln, bstate, hdr, roff, recl}));
			}
			drv.fetch(meta, dmeta, sizeof meta);
			c.skipped += meta[2] - 4 * n; // every consumed line is a skipped one or belongs to one of the n records
			drv.phase(FQS_P_COMPOSE);
			const bool go_on = n == 0 || visit(FqsWin{ln, recl, n});
			c.n_records += n;
			if (!go_on) return FS_OK;
		}
		// a file that is at its end and has no line left ends the input: an unterminated last line does not count, nor what the other file
		// still has, and the record the end cut off does not exist
		if ((end1 && L1 == L) || (end2 && L2 == L)) return FS_OK;
		if (meta[2] == 0) return FS_E_TOO_LARGE; // a file that goes on has a full window, and not one line pair of it could be consumed
		drv.phase(FQS_P_PARSE);
		for (int f = 0; f < 2; ++f) { // the carry to the other buffer's front
			const int64_t a = meta[f], left = have[f] - a;
			drv.items("fs_window", (left + 15) / 16, FsWindowF{win[f][cur] + a, left, win[f][cur ^ 1]});
			have[f] = left;
		}
		cur ^= 1;
	}
}

// ---- detection: the first of records 0 .. 199 whose header matches a pattern decides.  c.format, c.decided
template <class Drv, class Src> int fqs_detect(Drv &drv, Src &src, int64_t window, FqsCounts &c)
{
	c.format = FQS_UNKNOWN; c.decided = -1;
	return fqs_stream(drv, src, window, c, [&](const FqsWin &W) {
		const int64_t left = FQS_DETECT_RECORDS - c.n_records, m = W.n < left ? W.n : left;
		if (m <= 0 || m > FQS_DETECT_RECORDS) return false;
		uint8_t *cls = (uint8_t *)drv.work(FQS_W_CLASS, m);
		drv.items("fqs_match", m, FqsMatchF{W.ln, W.rec_line, cls});
		uint8_t h[FQS_DETECT_RECORDS];
		drv.fetch(h, cls, (size_t)m);
		for (int64_t i = 0; i < m; ++i)
			if (h[i]) { c.format = h[i]; c.decided = c.n_records + i; return false; }
		return c.n_records + W.n < FQS_DETECT_RECORDS;
	});
}

// ---- conversion: every record of what src delivers, rewritten for `format` (1 .. 3), to the sink slab by slab
template <class Drv, class Src, class Sink> int fqs_convert(Drv &drv, Src &src, int32_t format, int64_t window, int64_t slab_bytes, Sink &sink, FqsCounts &c)
{
	if (c.off1) c.off1->assign(1, 0);
	if (c.off2) c.off2->assign(1, 0);
	return fqs_stream(drv, src, window, c, [&](const FqsWin &W) {
		const int64_t n = W.n;
		FqsRec *fld = (FqsRec *)drv.work(FQS_W_FLD, (int64_t)sizeof(FqsRec) * n);
		int64_t *s1 = (int64_t *)drv.work(FQS_W_S1, 8 * n), *s2 = (int64_t *)drv.work(FQS_W_S2, 8 * n), *cnt = (int64_t *)drv.work(FQS_W_CNT, 8 * n);
		int64_t *o1 = (int64_t *)drv.work(FQS_W_O1, 8 * (n + 1)), *o2 = (int64_t *)drv.work(FQS_W_O2, 8 * (n + 1)), *cnto = (int64_t *)drv.work(FQS_W_CNTO, 8 * (n + 1));
		uint64_t *bcl = (uint64_t *)drv.work(FQS_W_BCL, 8 * n);
		drv.items("fqs_fields", n, FqsFieldsF{W.ln, W.rec_line, format, fld, s1, s2, cnt, bcl});
		drv.scan(s1, o1, n); drv.scan(s2, o2, n); drv.scan(cnt, cnto, n);
		const int64_t both = drv.get(&cnto[n]), longest_bc = (int64_t)drv.max64(bcl, n);
		c.with_bc += both & 0xffffffff; c.valid += both >> 32;
		if (longest_bc > c.max_bc) c.max_bc = longest_bc;
		const uint64_t big1 = drv.max64((const uint64_t *)s1, n), big2 = drv.max64((const uint64_t *)s2, n);
		const int64_t longest = (int64_t)(big1 > big2 ? big1 : big2), cap = slab_bytes > longest ? slab_bytes : longest;
		const int64_t all1 = drv.get(&o1[n]), all2 = drv.get(&o2[n]);
		for (int f = 0; f < 2; ++f)
			if (std::vector<int64_t> *v = f ? c.off2 : c.off1) {
				std::vector<int64_t> h((size_t)n + 1);
				drv.fetch(h.data(), f ? o2 : o1, (size_t)(n + 1) * 8);
				const int64_t base = f ? c.bytes2 : c.bytes1;
				for (int64_t r = 1; r <= n; ++r) v->push_back(base + h[(size_t)r]);
			}
		int64_t at1 = 0, at2 = 0; // o1[j0], o2[j0]
		for (int64_t j0 = 0; j0 < n;) {
			// the last j1 in (j0, n] at which both files' bytes still fit slab_bytes, or j0 + 1: one record always goes
			int64_t lo = j0 + 1, hi = n;
			if (all1 - at1 <= slab_bytes && all2 - at2 <= slab_bytes) lo = n; // the common case: the rest of the window is one slab
			while (lo < hi) {
				const int64_t mid = lo + (hi - lo + 1) / 2;
				if (drv.get(&o1[mid]) - at1 <= slab_bytes && drv.get(&o2[mid]) - at2 <= slab_bytes) lo = mid; else hi = mid - 1;
			}
			const int64_t e1 = drv.get(&o1[lo]), e2 = drv.get(&o2[lo]);
			uint8_t *d1 = nullptr, *d2 = nullptr;
			sink.take(c.slabs, cap, e1 - at1, e2 - at2, &d1, &d2);
			drv.items("fqs_compose", (lo - j0) * 2 * FS_GATHER_LANES, FqsComposeF{W.ln.t1, W.ln.t2, fld, o1, o2, j0, d1, d2});
			sink.give(c.slabs, j0, lo, e1 - at1, e2 - at2);
			++c.slabs;
			j0 = lo; at1 = e1; at2 = e2;
		}
		c.bytes1 += all1; c.bytes2 += all2;
		return true;
	});
}

} // namespace arx

// bam_records.h -- from the path's results to BAM records: the part of DumpToBams / AppendBam (src/aligner/bamwriter.go:283-568, 635-658)
// that turns the placed candidate of every read into a record, for a whole super-batch at a time, on host threads.  Host code of
// libarachne_amd.so (C ABI: arx_recbuf_* in include/arachne_amd.h); the sink that takes the records is bam_sink.h.
//
// Two modes over the same size / scan / fill passes.
//
// The rules of a record's fields -- the score rule and "unmapped", the active candidate, the flag word, MAPQ, TempLen, the CIGAR op table,
// which sets carry BX / VX -- are bam_rules.h's functions, shared by both modes here, the encoder (bam_sink.h) and the device (dev_records.h).
//
// arx_recbuf_build (kept as it was first written; tests/test_e2e.py pins it): one record per read, its ACTIVE candidate (bam_active), with
//   flags / pos / mapq / mate / template length  from bam_unmapped of the candidate and of its mate, both positions as the candidates hold
//              them (0-based already); an unmapped record has rid / pos -1 and mapq 0, an unmapped mate rid / pos -1
//   CIGAR      bam_cigar_word; read and qualities reversed for reverse-strand records (:372-375; reverseComp / reverseQual)
//   aux        RG:Z (the R1 header's last field, reader.go:144-153), AS:i (score), XM:Z:0, AM:Z:0|1, XT:C:0, and for a set with bam_set_bx
//              BX:Z + VX:C:1 (:555-559).
// That is NOT the reference's tag set: the reference never writes a read without mapq_data -- every Alignment is created with one
// (aligner.go:1601) and estimateMapQualities fills it for every barcode, with or without RFA (aligner.go:471, 496).  Its AS also is the
// BWA score rather than mapq_data.score, and its mate / TempLen rules read the mate's own is_proper.  Those stay as they are in this mode.
//
// arx_recbuf_build_full: the reference's record set.  Every read's primary record, then its split record (Alignment.secondary from
// arx_split: flag 0x100, TempLen 0, HardClip of :660-689 after the reverse-complement), with
//   flags / mate / TempLen  the same functions on positions AS MUTATED by AppendBam (:286-366): a record the score rule unmaps gets pos = -1, mapq = 0 before
//              anything is computed, and every record written later sees that -- read 2p is written before 2p+1, so 2p+1 sees its mate
//              at pos -1 (mate unmapped, TempLen 0), a split record's SA is left out when its primary was unmapped, and a forward primary
//              the rule unmaps while its mate stays mapped on the same contig gets TempLen mate.aend - (-1), the reference's form.  The
//              mate-unmapped test is the reference's: mate.pos == -1, or the score rule on the mate's score under the PRIMARY's is_proper.
//   aux        RG XS XC AC AS XM AM XT SA BX VX DM in the reference's order (:390-563), integers as `i` (auxify_int), strings NUL-ended.
//              XS / AS / XM / XT / XC's second best / DM's inputs come from arx_batch_tags; XC / AC list "ref,read,1;" per mismatch location
//              of the second best / the record's own alignment (arx_batch_post's lists); SA (:462-494) "contig,pos,strand,cigar,mapq,NM;"
//              with the raw BWA ops (reversed for '-', S printed as H only on the primary's SA), NM = mismatches + I/D lengths.
//              Split records: XS / AS = second_best2 / 2, score2 / 2 (truncated), XC empty, XM:Z:0, XT:i:0.
//   DM         written on primary records only.  A split candidate is never active, so the reference's molecule_difference on it is
//              whatever the FIRST setMoleculeDifferences call (aligner.go:483, before Optimize) left there, or 0; reproducing that needs a
//              snapshot taken inside the RFA kernel on the timed path.  Split records carry no DM here.
//   bucket     per record the position bucket of arx_bucket_table, chosen by IsUnmapped() (the score rule alone) as AppendBams does (:280).
// Left out in both modes: the -debug tags (:495-553), which no command-line path reaches.
//
// The device builds both record sets too, already BAM-encoded: arx_batch_records (dev_records.h) the first mode's, arx_batch_records_full
// (dev_records_full.h) the full mode's -- primary and split records, the whole tag set, the bucket of every record and a second stream grouped
// by bucket -- from what arx_batch_post and arx_batch_tags left in HBM.  What the full mode decides per read and per record (ReadState, the
// split record's flag and fields, order and length of the aux fields, SA's pieces, the bucket) is stated in bam_rules.h for both.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <thread>
#include <vector>
#include "../../include/arachne_amd.h"
#include "bam_rules.h"

namespace arx {

// CreateBAMs' files (bamwriter.go:134-188), in creation order; contig_file[i]: the file of contig i's first chunk
inline void bucket_table(int n_contigs, const char *const *names, const int32_t *lens, int64_t chunk, int32_t *contig_file, std::vector<std::string> &files)
{
	files.clear();
	int64_t running = 0;
	int32_t last = -1;
	char buf[64];
	for (int i = 0; i < n_contigs; ++i) {
		const int64_t len = lens[i], n_chunks = (len + chunk - 1) / chunk;
		snprintf(buf, sizeof buf, "%06d-", i);
		const std::string stem = std::string(buf) + names[i] + "_";
		if (n_chunks > 1) {
			contig_file[i] = (int32_t)files.size();
			for (int64_t k = 0; k < n_chunks; ++k) { snprintf(buf, sizeof buf, "%010lld", (long long)(k * chunk)); files.push_back(stem + buf + "_pos_bucketed.bam"); }
		} else {
			if (running == 0 || running + len > chunk) { last = (int32_t)files.size(); files.push_back(stem + "0000000000_pos_bucketed.bam"); running = len; }
			else running += len;
			contig_file[i] = last;
		}
	}
	files.push_back("ZZZ_unmapped_pos_bucketed.bam");
}

// aux bytes of the full mode, counted (p == null) or written
struct AuxOut {
	uint8_t *p; int64_t n = 0;
	void put(const void *s, size_t l) { if (p) memcpy(p + n, s, l); n += (int64_t)l; }
	void tag(const char *t, char type) { const char h[3] = {t[0], t[1], type}; put(h, 3); }
	void i32(const char *t, int32_t v) { tag(t, 'i'); put(&v, 4); }
	void z(const char *t, const char *s, size_t l) { tag(t, 'Z'); put(s, l); put("", 1); }
	void zs(const char *t, const std::string &s) { z(t, s.data(), s.size()); }
};

struct RecBuf {
	std::vector<int64_t> name_off, cigar_off, seq_off, aux_off;
	std::vector<char> names;
	std::vector<int32_t> flag, rid, pos, mate_rid, mate_pos, tlen;
	std::vector<uint8_t> mapq, seq, qual, aux;
	std::vector<uint32_t> cigars;
	std::vector<int32_t> act; // active candidate of every read
	std::vector<int64_t> rbase; // full mode: record of every read's primary (its split record follows it)
	std::vector<int32_t> bucket; // full mode: position bucket of every record

	// What AppendBam sees when it writes read r's records (full mode): bam_rules.h's, shared with the device (dev_records_full.h)
	template <class C> static inline bool pair_at(const C &a, int64_t apos, const C &b, int64_t bpos) { return bam_pair_at(a, apos, b, bpos); }
	typedef BamReadState ReadState;

	// sb: the super-batch the batch was created from; cand_off / cands: arx_batch_rfa_fetch; alns / cigars: arx_batch_fetch (cands[].reg indexes
	// them); post: arx_batch_post_fetch's per-candidate records or NULL (then no duplicate flags); full: null for arx_recbuf_build's record set
	bool build(const arx_super_batch &sb, const int32_t *cand_off, const arx_cand *cands, const arx_aln *alns, const uint32_t *cigs, const arx_cand_post *post,
	           int threads, arx_bam_batch *view, std::string &err, const arx_recbuf_full *full = nullptr)
	{
		const int64_t NP = sb.n_pairs, NR = 2 * NP;
		if (threads < 1) threads = 1;
		act.assign((size_t)NR, -1);
		// records: one per read, and in the full mode the split record right behind its primary
		rbase.assign((size_t)NR + 1, 0);
		for (int64_t r = 0; r < NR; ++r) rbase[(size_t)r + 1] = rbase[(size_t)r] + 1 + (full && full->split[r].split >= 0 ? 1 : 0);
		const int64_t NRec = rbase[(size_t)NR];
		name_off.assign((size_t)NRec + 1, 0); cigar_off.assign((size_t)NRec + 1, 0); seq_off.assign((size_t)NRec + 1, 0); aux_off.assign((size_t)NRec + 1, 0);
		flag.resize((size_t)NRec); rid.resize((size_t)NRec); pos.resize((size_t)NRec); mate_rid.resize((size_t)NRec); mate_pos.resize((size_t)NRec); tlen.resize((size_t)NRec); mapq.resize((size_t)NRec);
		if (full) bucket.assign((size_t)NRec, 0);
		std::vector<int64_t> base_off((size_t)NR + 1, 0), pair_set((size_t)NP);
		for (int64_t r = 0; r < NR; ++r) base_off[(size_t)r + 1] = base_off[(size_t)r] + sb.lens[r];
		for (int s = 0; s < sb.n_sets; ++s) for (int64_t p = sb.set_pair_off[s]; p < sb.set_pair_off[s + 1]; ++p) pair_set[(size_t)p] = s;
		std::vector<uint8_t> set_bx((size_t)sb.n_sets, 0);
		for (int s = 0; s < sb.n_sets; ++s) set_bx[(size_t)s] = bam_set_bx(sb.unique[s], sb.barcodes + sb.barcode_off[s], sb.barcode_off[s + 1] - sb.barcode_off[s]);
		bool bad = false;
		auto par = [&](auto fn) {
			std::vector<std::thread> th;
			for (int t = 0; t < threads; ++t) th.emplace_back([&, t]() { const int64_t lo = NR * t / threads, hi = NR * (t + 1) / threads; for (int64_t r = lo; r < hi; ++r) fn(r); });
			for (auto &x : th) x.join();
		};
		auto state = [&](int64_t r) { return bam_read_state(cands, alns, cigs, act[(size_t)r], act[(size_t)(r ^ 1)], full->split[r], r); }; // full mode
		// "ref,read,1;" per mismatch location of candidate i (XC / AC)
		auto mm_string = [&](int i) {
			std::string out;
			if (i < 0) return out;
			char b[48];
			for (int k = 0; k < post[i].n_mm; ++k) { snprintf(b, sizeof b, "%d,%d,1;", full->mm_ref[post[i].mm_off + k], full->mm_read[post[i].mm_off + k]); out += b; }
			return out;
		};
		// SA:Z pointing at candidate i written at position p with MAPQ q; hard: S printed as H (the primary's SA, :478-480)
		auto sa_string = [&](int i, int64_t p, int q, bool hard) {
			const arx_cand &x = cands[i];
			const arx_aln &al = alns[x.reg];
			std::string out = (x.rid >= 0 && x.rid < full->n_contigs) ? full->contig_names[x.rid] : "";
			char b[48];
			snprintf(b, sizeof b, ",%lld,%c,", (long long)p, x.reversed ? '-' : '+'); out += b;
			for (int k = 0; k < al.n_cigar; ++k) {
				const uint32_t w = bam_sa_word(cigs + al.cigar_off, al.n_cigar, k, x.reversed != 0);
				snprintf(b, sizeof b, "%u%c", w >> 4, bam_sa_op(w, hard)); out += b;
			}
			snprintf(b, sizeof b, ",%d,%d;", q, bam_sa_nm(post[i].n_mm, cigs + al.cigar_off, al.n_cigar)); out += b;
			return out;
		};
		// the aux fields of read r's primary (split = false) or split record (full mode), counted (bam_full_aux_len) or written in that order
		auto full_aux = [&](int64_t r, const ReadState &st, bool split, AuxOut &o) {
			const int64_t p = r >> 1; const int s = (int)pair_set[(size_t)p];
			const arx_read_tags &T = full->tags[r];
			const arx_split &S = full->split[r];
			const arx_cand &x = cands[split ? st.s : st.a];
			const int64_t rgl = sb.rg_off[p + 1] - sb.rg_off[p];
			const bool bx = set_bx[(size_t)s] != 0;
			int32_t xs, as, xt; bool xm;
			bam_full_ints(split, T, S, &xs, &as, &xt, &xm);
			const std::string xc = split ? std::string() : mm_string(T.second_best), ac = mm_string(split ? st.s : st.a);
			std::string sa, dm;
			const bool has_sa = bam_has_sa(split, st), has_dm = bam_has_dm(split, bx, x.active_molecule != 0, T.dm_n);
			if (has_sa) { int i; int64_t sp; int32_t q; bool hard; bam_sa_source(split, st, cands, S, &i, &sp, &q, &hard); sa = sa_string(i, sp, q, hard); }
			if (has_dm) {
				char b[64];
				const int l = snprintf(b, sizeof b, "%.6f", (double)T.dm_sum / (double)T.dm_n); // strconv.FormatFloat(x, 'f', 6, 64)
				dm.assign(b, (size_t)l);
			}
			const int64_t bcl = sb.barcode_off[s + 1] - sb.barcode_off[s];
			if (!o.p) {
				o.n = bam_full_aux_len(BamFullAux{(int32_t)rgl, (int32_t)xc.size(), (int32_t)ac.size(), has_sa ? (int32_t)sa.size() : -1, (int32_t)bcl, has_dm ? (int32_t)dm.size() : -1, bx});
				return;
			}
			for (int f = 0; f < FA_N; ++f) switch (f) {
			case FA_RG: if (rgl > 0) o.z("RG", sb.rgs + sb.rg_off[p], (size_t)rgl); break;
			case FA_XS: o.i32("XS", xs); break;
			case FA_XC: o.zs("XC", xc); break;
			case FA_AC: o.zs("AC", ac); break;
			case FA_AS: o.i32("AS", as); break;
			case FA_XM: o.z("XM", xm ? "1" : "0", 1); break;
			case FA_AM: o.z("AM", x.active_molecule ? "1" : "0", 1); break;
			case FA_XT: o.i32("XT", xt); break;
			case FA_SA: if (has_sa) o.zs("SA", sa); break;
			case FA_BX: if (bx) o.z("BX", sb.barcodes + sb.barcode_off[s], (size_t)bcl); break;
			case FA_VX: if (bx) o.i32("VX", 1); break;
			case FA_DM: if (has_dm) o.zs("DM", dm); break;
			}
		};
		// pass 1: the active candidate and the sizes of every record
		par([&](int64_t r) {
			int a = bam_active(cands, cand_off, r); // exactly one per read
			if (a < 0) { bad = true; a = cand_off[r]; }
			act[(size_t)r] = a;
		});
		if (bad) { err = "a read without an active candidate: arx_batch_rfa must have run on this batch"; return false; }
		if (full) for (int64_t r = 0; r < NR; ++r) {
			const int sp = full->split[r].split;
			if (!bam_split_ok(cands, cand_off, r, sp)) { err = ARX_BAM_SPLIT_TEXT; return false; }
		}
		par([&](int64_t r) {
			const int64_t q = rbase[(size_t)r];
			const arx_cand &c = cands[act[(size_t)r]];
			const int64_t p = r >> 1; const int s = (int)pair_set[(size_t)p];
			name_off[(size_t)q + 1] = sb.name_off[p + 1] - sb.name_off[p];
			cigar_off[(size_t)q + 1] = c.reg >= 0 ? alns[c.reg].n_cigar : 0;
			seq_off[(size_t)q + 1] = sb.lens[r];
			if (!full) {
				aux_off[(size_t)q + 1] = bam_first_aux_len(sb.rg_off[p + 1] - sb.rg_off[p], set_bx[(size_t)s] != 0, sb.barcode_off[s + 1] - sb.barcode_off[s]);
				return;
			}
			const ReadState st = state(r);
			AuxOut o{nullptr};
			full_aux(r, st, false, o);
			aux_off[(size_t)q + 1] = o.n;
			if (st.s >= 0) {
				name_off[(size_t)q + 2] = name_off[(size_t)q + 1];
				cigar_off[(size_t)q + 2] = alns[cands[st.s].reg].n_cigar;
				const int64_t kept = (int64_t)sb.lens[r] - st.hc0 - st.hc1;
				seq_off[(size_t)q + 2] = kept > 0 ? kept : 0;
				AuxOut o2{nullptr};
				full_aux(r, st, true, o2);
				aux_off[(size_t)q + 2] = o2.n;
			}
		});
		for (int64_t q = 0; q < NRec; ++q) { name_off[(size_t)q + 1] += name_off[(size_t)q]; cigar_off[(size_t)q + 1] += cigar_off[(size_t)q]; seq_off[(size_t)q + 1] += seq_off[(size_t)q]; aux_off[(size_t)q + 1] += aux_off[(size_t)q]; }
		names.resize((size_t)name_off[(size_t)NRec] + 1); cigars.resize((size_t)cigar_off[(size_t)NRec] + 1); seq.resize((size_t)seq_off[(size_t)NRec] + 1); qual.resize((size_t)seq_off[(size_t)NRec] + 1);
		aux.resize((size_t)aux_off[(size_t)NRec] + 1);
		// pass 2: fill
		static const char comp[5] = {'T', 'G', 'C', 'A', 'N'}, fwd[5] = {'A', 'C', 'G', 'T', 'N'};
		// name, CIGAR (BAM codes; S -> H at both ends for a split record), bases and qualities of record q from candidate x of read r
		auto fill_body = [&](int64_t r, int64_t q, const arx_cand &x, int hc0, int hc1, bool hard) {
			const int64_t p = r >> 1;
			memcpy(names.data() + name_off[(size_t)q], sb.names + sb.name_off[p], (size_t)(sb.name_off[p + 1] - sb.name_off[p]));
			if (x.reg >= 0) {
				const arx_aln &al = alns[x.reg];
				uint32_t *dst = cigars.data() + cigar_off[(size_t)q];
				for (int k = 0; k < al.n_cigar; ++k) dst[k] = bam_cigar_word(cigs[al.cigar_off + k]);
				if (hard) for (int k = 0; k < al.n_cigar; ++k) dst[k] = bam_hard_word(dst[k], k, al.n_cigar);                        // HardClip (:660-689)
			}
			const int L = sb.lens[r];
			const uint8_t *b = sb.bases + base_off[(size_t)r]; const char *qs = sb.quals + base_off[(size_t)r];
			uint8_t *so = seq.data() + seq_off[(size_t)q], *qo = qual.data() + seq_off[(size_t)q];
			const int lo = hc0, hi = L - hc1;
			for (int k = lo; k < hi; ++k) {
				if (x.reversed) { const uint8_t y = b[L - 1 - k]; so[k - lo] = (uint8_t)comp[y > 4 ? 4 : y]; qo[k - lo] = (uint8_t)qs[L - 1 - k]; }
				else { const uint8_t y = b[k]; so[k - lo] = (uint8_t)fwd[y > 4 ? 4 : y]; qo[k - lo] = (uint8_t)qs[k]; }
			}
		};
		// the fixed fields of record q: candidate x written at xpos (-1: unmapped) with MAPQ mq, its mate m at mpos
		auto put_fields = [&](int64_t q, uint32_t fl, const arx_cand &x, int64_t xpos, int32_t mq, bool mate_un, const arx_cand &m, int64_t mpos, int32_t tl) {
			const BamFields f = bam_fields(x, xpos, mq, mate_un, m, mpos);
			flag[(size_t)q] = (int32_t)fl; rid[(size_t)q] = f.rid; pos[(size_t)q] = f.pos; mapq[(size_t)q] = (uint8_t)f.mapq;
			mate_rid[(size_t)q] = f.mate_rid; mate_pos[(size_t)q] = f.mate_pos; tlen[(size_t)q] = tl;
		};
		par([&](int64_t r) {
			const int64_t q = rbase[(size_t)r];
			const arx_cand &c = cands[act[(size_t)r]], &m = cands[act[(size_t)(r ^ 1)]];
			const int64_t p = r >> 1; const int s = (int)pair_set[(size_t)p];
			if (full) {
				const ReadState st = state(r);
				put_fields(q, bam_flag(r & 1, c.is_proper, st.cpos == -1, st.mate_un, m.reversed, c.reversed, post[st.a].duplicate, false), c, st.cpos, c.mapq, st.mate_un, m, st.mpos,
				           bam_tlen(c, m, st.cpos, st.mpos));
				bucket[(size_t)q] = bam_bucket(bam_score_rule(c), c.rid, c.pos, full->contig_file, full->n_contigs, full->chunk, full->unmapped_file);
				fill_body(r, q, c, 0, 0, false);
				AuxOut o{aux.data() + aux_off[(size_t)q]};
				full_aux(r, st, false, o);
				if (st.s >= 0) {
					const arx_cand &x = cands[st.s];
					const arx_split &S = full->split[r];
					put_fields(q + 1, bam_split_flag(r & 1, S.is_proper != 0, x, st, m, post[st.s].duplicate != 0), x, st.spos, S.mapq, st.mate_un, m, st.mpos, 0);
					bucket[(size_t)q + 1] = bam_bucket(st.spos == -1, x.rid, x.pos, full->contig_file, full->n_contigs, full->chunk, full->unmapped_file);
					fill_body(r, q + 1, x, st.hc0, st.hc1, true);
					AuxOut o2{aux.data() + aux_off[(size_t)q + 1]};
					full_aux(r, st, true, o2);
				}
				return;
			}
			const bool un = bam_unmapped(c), mun = bam_unmapped(m);
			put_fields(q, bam_flag(r & 1, c.is_proper, un, mun, m.reversed, c.reversed, post && post[act[(size_t)r]].duplicate, false), c, un ? -1 : c.pos, c.mapq, mun, m, m.pos,
			           bam_tlen(c, m, c.pos, m.pos));
			fill_body(r, q, c, 0, 0, false);
			AuxOut o{aux.data() + aux_off[(size_t)q]};
			const int64_t rgl = sb.rg_off[p + 1] - sb.rg_off[p];
			if (rgl > 0) o.z("RG", sb.rgs + sb.rg_off[p], (size_t)rgl);
			o.i32("AS", c.score); o.z("XM", "0", 1); o.z("AM", c.active_molecule ? "1" : "0", 1); o.tag("XT", 'C'); o.put("", 1);
			if (set_bx[(size_t)s]) { o.z("BX", sb.barcodes + sb.barcode_off[s], (size_t)(sb.barcode_off[s + 1] - sb.barcode_off[s])); o.tag("VX", 'C'); o.put("\1", 1); }
		});
		view->n_records = NRec;
		view->name_off = name_off.data(); view->names = names.data(); view->flag = flag.data(); view->rid = rid.data(); view->pos = pos.data(); view->mapq = mapq.data();
		view->mate_rid = mate_rid.data(); view->mate_pos = mate_pos.data(); view->tlen = tlen.data(); view->cigar_off = cigar_off.data(); view->cigars = cigars.data();
		view->seq_off = seq_off.data(); view->seq = seq.data(); view->qual = qual.data(); view->qual_offset = 33; view->aux_off = aux_off.data(); view->aux = aux.data();
		return true;
	}
};

} // namespace arx

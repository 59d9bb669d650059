"""Shared by tests/test_device_records_full.py (host double) and tests/test_device_records_full_gpu.py (product library): a crafted FASTQ
workload for the full records phase (arx_batch_records_full) on two contigs of 300 kb and 60 kb, the HOST path that is the reference of every
comparison -- arx_recbuf_build_full -> arx_bam_write on a host writer for the stream, arx_bam_write_select into a writer of its own for
every bucket, the files inflated -- and the identity check both suites run."""
import os
import types

import numpy as np

from arachne_amd import api, synth
import reccases as rc

CHUNK = 100000
NOT_UNIQUE = {"AAAT-1"}


def make_genome():
    """300 kb + 60 kb, contig names of 1 and 27 bytes, and a 3 kb stretch of the first contig planted a second time, 2 % diverged, in the
    second: a read drawn from the original has the copy as its second best, with mismatches to list in XC"""
    g = synth.make_genome(31, [300000, 60000])
    for s in g.seqs:
        s[s > 3] = 0
    g.names = ["c", "chrS2_a_longer_contig_name"]
    rng = np.random.default_rng(5)
    seg = g.seqs[0][120000:123000].copy()
    hit = rng.random(len(seg)) < 0.02
    seg[hit] = (seg[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    g.seqs[1][20000:23000] = seg
    return g


def crafted_pairs(g, seed=9):
    """reccases.crafted_pairs on the first 190 kb of the first contig (its last chunk stays empty), then a barcode of what only the full record
    set shows: chimeric reads on both strands and in both orders, one with a deletion beside the junction, reads with 1 and 6 substitutions,
    reads from the planted original, a 30-base read whose mate maps alone, pairs on the second contig, a molecule's worth of pairs for DM"""
    rng = np.random.default_rng(seed)
    G, H = g.seqs[0], g.seqs[1]
    out = rc.crafted_pairs(types.SimpleNamespace(seqs=[G[:190000]]))
    k = [0]

    def name(n=12):
        k[0] += 1
        return ("%dz" % k[0] + "m" * n)[:n]

    sp = []
    for i in range(6):                                                          # R1 = 80 bases at A + 70 bases 50 kb on; the mate next to A
        A = int(rng.integers(5000, 100000))
        B = A + 50000
        r1 = np.concatenate([G[A:A + 80], G[B + 80:B + 150]])
        r2 = rc._rc(G[A + 200:A + 350])
        sp.append((r1, r2) if i & 1 == 0 else (rc._rc(r1), G[A - 300:A - 150].copy()))   # ... and on the other strand
    for i in range(6):                                                          # the mate next to the SECOND part: the first part is the split
        A = int(rng.integers(5000, 100000))
        B = A + 50000
        r1 = np.concatenate([G[A:A + 70], G[B + 70:B + 150]])
        r2 = rc._rc(G[B + 300:B + 450])
        sp.append((r1, r2) if i & 1 == 0 else (rc._rc(r1), G[B - 300:B - 150].copy()))
    for i in range(4):                                                          # a deletion of 4 bases inside the part the mate stands next to
        A = int(rng.integers(5000, 100000))
        B = A + 40000
        r1 = np.concatenate([G[A:A + 60], G[A + 64:A + 124], G[B:B + 90]])
        sp.append((r1, rc._rc(G[A + 300:A + 450])))
    for n_sub in (1, 6, 9):                                                     # AC lists of 1 and 5+ entries
        A = int(rng.integers(5000, 100000))
        r1 = G[A:A + 150].copy()
        for j in range(n_sub):
            r1[10 + 14 * j] = (r1[10 + 14 * j] + 1) % 4
        sp.append((r1, rc._rc(G[A + 250:A + 400])))
    for i in range(4):                                                          # from the planted original: the copy is the second best
        A = 120200 + 500 * i
        sp.append((G[A:A + 150].copy(), rc._rc(G[A + 250:A + 400])))
    for i in range(3):                                                          # 30 bases whose mate maps 20 kb away: unmapped by the score rule, the mate stays
        A = 30000 + 7000 * i
        sp.append((G[A:A + 30].copy(), rc._rc(G[A + 20000:A + 20150])))
    for i in range(6):                                                          # the second contig
        A = int(rng.integers(1000, 15000)) if i < 3 else int(rng.integers(30000, 55000))
        sp.append((H[A:A + 150].copy(), rc._rc(H[A + 200:A + 350])))
    out += [("AACC-1", name(8 + i % 7), "rgE", r1, r2) for i, (r1, r2) in enumerate(sp)]
    mol = []
    for i in range(30):                                                         # one molecule: 30 pairs inside 25 kb, a few with a substitution
        A = 150000 + int(rng.integers(0, 25000))
        r1 = G[A:A + 150].copy()
        if i % 3 == 0:
            r1[75] = (r1[75] + 2) % 4
        mol.append((r1, rc._rc(G[A + 220:A + 370])))
    out += [("AAGG-1", name(10), "rgF", r1, r2) for r1, r2 in mol]
    return out


class World:
    """index, FASTQ files, reference and the whole workload as one super-batch"""

    def __init__(self, lib_path, d):
        self.lib_path, self.d = lib_path, d
        self.g = make_genome()
        self.fa = rc.make_index(d, self.g, lib_path)
        self.pairs = crafted_pairs(self.g)
        self.files = (os.path.join(d, "c1.fq"), os.path.join(d, "c2.fq"))
        rc.write_fastq(self.pairs, *self.files)
        self.ref = api.Reference(self.fa, lib_path=lib_path)
        self.names, _, self.clens, _, _ = self.ref.contigs()
        self.table = api.bucket_table(self.names, self.clens, CHUNK, lib_path=lib_path)
        self.fd = api.Feeder(*self.files, lib_path=lib_path)
        sb, self.v = self.fd.next_raw(10 ** 6)
        assert int(self.v["n_pairs"]) == len(self.pairs)
        self.sb, self.keep = rc.with_unique(sb, self.v, NOT_UNIQUE)

    def close(self):
        self.fd.close()
        self.ref.close()


class FullCase:
    """One super-batch taken through the path on `ref` up to where both record paths start (run, rfa, post and tags done, everything home),
    and the host path's results: the view, the bucket of every record, the inflated stream file and every bucket's inflated file body"""

    def __init__(self, ref, sb, v, table, lib_path, d, tag, penalty=-4):
        self.ref, self.sb, self.v, self.table = ref, sb, v, table
        self.batch = ref.batch(v["bases"], v["lens"]).run()
        self.batch.rfa(v["set_pair_off"], v["do_rfa"], penalty=penalty, fetch=False)
        self.buf = {}
        self.batch.fetch_into(self.buf)
        self.post = self.batch.post()
        self.tags = self.batch.tags()
        self.rb = api.RecBuf(lib_path=lib_path)
        b = self.buf
        self.view, self.bucket = self.rb.build_full(sb, b["cand_off"], b["cands"], b["alns"], b["cigars"], self.post["post"], self.post["split"], self.post["mm_ref"],
                                                    self.post["mm_read"], self.tags, table, threads=2)
        names, _, clens, _, _ = ref.contigs()

        def writer(path):
            return api.BamWriter(path, names, clens, extra_header="@PG\tID:t\n", threads=2, level=1, lib_path=lib_path)
        p = os.path.join(d, tag + "_stream.bam")
        w = writer(p)
        w.write_view(self.view)
        w.close()
        data = rc.inflate(p)
        self.header = data[:rc.header_len(data)]
        self.stream = data[len(self.header):]
        self.order = np.argsort(self.bucket, kind="stable")
        cuts = np.searchsorted(self.bucket[self.order], np.arange(len(table.files) + 1))
        self.bucket_body = []
        for f in range(len(table.files)):
            p = os.path.join(d, tag + "_bucket%d.bam" % f)
            w = writer(p)
            if cuts[f + 1] > cuts[f]:
                w.write_select(self.view, self.order[cuts[f]:cuts[f + 1]])
            w.close()
            self.bucket_body.append(rc.inflate(p)[len(self.header):])
        self.cuts = cuts

    def free(self):
        self.batch.free()
        self.rb.free()


def check_identity(c):
    """arx_batch_records_full on the case's batch against the host path: the stream, the record offsets, the buckets, every bucket's slice of the
    grouped stream, both offset tables.  -> (n_records, n_bytes)"""
    n, nb = c.batch.records_full(c.sb, c.table)
    assert (n, nb) == (len(c.bucket), len(c.stream))
    stream, off = c.batch.records_fetch()
    assert stream.tobytes() == c.stream
    assert np.array_equal(off, rc.walk(c.stream)[0])
    g = c.batch.records_buckets_fetch()
    assert np.array_equal(g["bucket"], c.bucket)
    assert np.array_equal(g["rec_off"], c.cuts)
    size = np.diff(off)
    want_byte = np.concatenate([[0], np.cumsum(size[c.order])])[c.cuts]
    assert np.array_equal(g["byte_off"], want_byte)
    grouped = g["grouped"].tobytes()
    for f, body in enumerate(c.bucket_body):
        assert grouped[g["byte_off"][f]:g["byte_off"][f + 1]] == body, c.table.files[f]
    assert len(grouped) == nb == g["byte_off"][-1]
    return n, nb


def e2e_paths(st, layout, out):
    """the files of a finished e2e.run(..., out, layout=layout) with stats st: name ("k.bam" for worker k's file) -> path"""
    if layout == "reference":
        return {f: os.path.join(out, f) for f in st["files"]}
    return {f"{k}.bam": f"{out}.{k}.bam" for k in range(st["workers"])}


def records_of(path):
    """the records of a BAM file as a list of their bytes"""
    data = rc.inflate(path)
    s = data[rc.header_len(data):]
    off = rc.walk(s)[0]
    return [s[off[i]:off[i + 1]] for i in range(len(off) - 1)]

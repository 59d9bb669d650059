"""Shared by tests/test_bam_index_feeds_sim.py (the host program over the push form of arachne_amd/csrc/dev_bamindex.h) and
tests/test_bam_index_feeds_gpu.py (the product's kernels through arx_selftest_bam_index_feeds and the indexing writer): the record streams of
baicases.py and csicases.py laid out the way a writer lays its file out, and streams of more than one BGZF block that put records, fields and
runs at the blocks' edges.  Nothing here comes from the code under test: the expected bytes are baicases.bai_of and csicases.csi_of over the
writer's layout, stated here from the text of the issue --
  the header's H bytes end their own ceil(H / 65280) blocks, every block behind them holds 65280 bytes of the record stream but the last --
with file offsets whose steps are anything in 26 .. 65536, so that a block's ordinal taken for its offset shows.
  relaid(case, min_shift) -> Laid     min_shift None: the .bai
  cuttings(laid)                      {name: feed ends}: one feed, one per record, feeds of 7 and of 61 bytes
  edges() -> {name: Laid}             the block-edge cases; check_edges() asserts from the bytes that each is what its name claims"""
import functools
import struct

import baicases as bc
import csicases as cc
from baicases import m
from sortcases import filler, rec

BLOCK = 65280


def layout(hdr, n_bytes):
    """the inflated sizes of a writer's blocks, the EOF block not among them"""
    sizes = [min(BLOCK, hdr - o) for o in range(0, hdr, BLOCK)]
    return sizes + [min(BLOCK, n_bytes - o) for o in range(hdr, n_bytes, BLOCK)]


def irregular_at(n_blocks, seed):
    """n_blocks + 1 file offsets (the last: the EOF block's); the steps a fixed scramble over 26 .. 65536, the smallest and the largest among them"""
    at, x = [seed % 9973], seed * 2654435761 % (1 << 32)
    for b in range(n_blocks):
        x = (x * 1103515245 + 12345) % (1 << 31)
        at.append(at[-1] + (26 if b % 5 == 1 else 65536 if b % 5 == 3 else 26 + x % (65536 - 25)))
    return at


class Laid:
    """a record stream behind hdr bytes of header in a writer's layout, with the index the contract asks for (want) or the refusal"""
    def __init__(self, recs, ref_len, hdr=0, min_shift=None, seed=1, stream=None):
        self.recs, self.ref_len, self.hdr, self.min_shift = list(recs), list(ref_len), hdr, min_shift
        self.stream = bytes(0xEE for _ in range(hdr)) + b"".join(self.recs) if stream is None else stream
        self.isize = layout(hdr, len(self.stream))
        self.at = irregular_at(len(self.isize), seed + len(self.stream))
        self.off = [hdr]
        for r in self.recs:
            self.off.append(self.off[-1] + len(r))
        try:
            if min_shift is None:
                self.want = bc.bai_of(self.recs, hdr, self.ref_len, self.at, self.isize)
            else:
                self.want = cc.csi_of(self.recs, hdr, self.ref_len, self.at, self.isize, min_shift)
            self.refused = None
        except bc.Refused as e:
            self.want, self.refused = None, e
        except AssertionError:                                   # a stream that is no list of records (baicases.broken): neither
            self.want, self.refused = None, None

    def packed(self):
        """the case file of tests/bixsim/bam_index_feeds_sim.cpp (that of tests/baisim)"""
        words = [len(self.stream), self.hdr, len(self.ref_len), len(self.isize)] + self.ref_len + self.at + self.isize
        return struct.pack("<%dq" % len(words), *words) + self.stream


def relaid(case, min_shift=None, seed=1):
    return Laid(case.recs, case.ref_len, case.hdr, min_shift, seed, stream=case.stream)


def cuttings(k, sizes=(7, 61)):
    n = len(k.stream)
    out = {"one": [n], "record": sorted(set(o for o in k.off[1:] if o < n) | {n})}
    for s in sizes:
        out["by%d" % s] = list(range(k.hdr + s, n, s)) + [n]
    return out


def feeds_packed(groups):
    """the feeds file of the host program"""
    words = []
    for ends in groups:
        words += [len(ends)] + list(ends)
    return struct.pack("<%dq" % len(words), *words)


# ---- the block-edge cases: record streams above one block.  Big records (filler: exactly so many bytes) bring the stream to the edge
def _upto(target, pos0=10, size=4000, rid=0):
    """records of contig rid that fill exactly `target` bytes; positions ascend from pos0"""
    out, left, k = [], target, 0
    while left > 0:
        s = size if left >= size + 38 else left
        out.append(filler(s, rid, pos0 + k, b"f"))
        left -= s
        k += 1
    assert sum(len(r) for r in out) == target
    return out


@functools.lru_cache(maxsize=None)
def edges():
    c = {}
    ref = [1 << 20, 1 << 20]
    small = lambda p, name=b"s", rid=0: m(rid, p, name)
    c["start_at_boundary"] = Laid(_upto(BLOCK) + [small(500), small(501)], ref)
    c["straddles_boundary"] = Laid(_upto(BLOCK - 20) + [small(500), small(501)], ref, hdr=33)
    c["block_size_cut"] = Laid(_upto(BLOCK - 2) + [small(500), small(501)], ref, hdr=33)
    c["total_two_blocks"] = Laid(_upto(2 * BLOCK), ref)
    c["total_two_blocks_plus_1"] = Laid(_upto(2 * BLOCK - 38) + [filler(39, 0, 900)], ref)
    c["header_65280"] = Laid(_upto(BLOCK + 100), ref, hdr=BLOCK)
    c["header_65281"] = Laid(_upto(BLOCK + 100), ref, hdr=BLOCK + 1)
    # two runs of one leaf bin (window 1) with a run of its parent between them: the earlier run ends and the later begins in one block, or in neighbours
    a, mid, b = [small(20000, b"a0"), small(20010, b"a1")], [m(0, 20020, b"parent", "20000M")], [small(20030, b"b0"), small(20040, b"b1")]
    lead = _upto(BLOCK + 500, pos0=10)                                    # all of them in block 1
    c["runs_joined_in_one_block"] = Laid(lead + a + mid + b, ref)
    n_a, n_mid = sum(len(r) for r in a), len(mid[0])
    lead2 = _upto(BLOCK - n_a - n_mid + 5, pos0=10)                      # the parent straddles the boundary: a ends in block 0, b begins in block 1
    c["runs_apart_in_neighbours"] = Laid(lead2 + a + mid + b, ref)
    same = [m(0, 30000 + j, b"r%d" % j, l_seq=100) for j in range(40)]    # one run of forty records
    c["run_across_feeds"] = Laid(same, ref, hdr=12)
    c["run_across_pieces"] = Laid(same, ref, hdr=12)
    c["zero_records"] = Laid([], ref, hdr=BLOCK + 7)
    c["only_unplaced"] = Laid([filler(3000, -1, -1, b"u") for _ in range(30)], ref, hdr=12)
    return c


def edge_cuttings(name, k):
    """what the edge cases are cut into: one feed, one per record, and feeds of a size that is no divisor of anything here"""
    out = cuttings(k, sizes=(4099,))
    if name == "run_across_feeds":
        out["by61"] = cuttings(k, sizes=(61,))["by61"]
    return out


def check_edges():
    c = edges()
    rel = lambda k, o: (o - k.hdr) % BLOCK                               # where a byte of the stream lies in its block
    k = c["start_at_boundary"]
    assert rel(k, k.off[-3]) == 0 and k.off[-3] - k.hdr == BLOCK
    k = c["straddles_boundary"]
    assert k.off[-3] - k.hdr == BLOCK - 20 and k.off[-2] - k.hdr > BLOCK
    k = c["block_size_cut"]
    assert k.off[-3] - k.hdr == BLOCK - 2
    assert len(c["total_two_blocks"].stream) == 2 * BLOCK and len(c["total_two_blocks_plus_1"].stream) == 2 * BLOCK + 1
    assert c["total_two_blocks"].isize == [BLOCK, BLOCK] and c["total_two_blocks_plus_1"].isize == [BLOCK, BLOCK, 1]
    assert c["header_65280"].isize[:2] == [BLOCK, BLOCK] and c["header_65281"].isize[:3] == [BLOCK, 1, BLOCK]
    one, two = bc.read_bai(c["runs_joined_in_one_block"].want)["refs"][0]["bins"], bc.read_bai(c["runs_apart_in_neighbours"].want)["refs"][0]["bins"]
    assert len(one[4682]) == 1 and len(two[4682]) == 2 and 585 in one and 585 in two
    k = c["runs_apart_in_neighbours"]
    assert k.off[-4] - k.hdr < BLOCK < k.off[-3] - k.hdr               # the parent: starts in block 0, ends in block 1
    k = c["run_across_feeds"]
    assert len({bc.reg2bin(*bc.interval(r)) for r in k.recs}) == 1 and len(k.stream) > 40 * 61
    assert c["zero_records"].recs == [] and c["zero_records"].isize == [BLOCK, 7]
    assert all(bc.fields(r)[1] == -1 for r in c["only_unplaced"].recs) and bc.read_bai(c["only_unplaced"].want)["n_no_coor"] == 30
    for name, k in c.items():
        assert k.refused is None and len(k.stream) < 1 << 20, name
        if name not in ("run_across_feeds", "run_across_pieces"):
            assert len(k.stream) > BLOCK, name
        assert min(b - a for a, b in zip(k.at, k.at[1:])) >= 26 and max(b - a for a, b in zip(k.at, k.at[1:])) <= 65536

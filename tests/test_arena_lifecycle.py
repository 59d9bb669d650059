"""The lifetime of a batch's work memory: one handle driven through run, rfa, post and tags, each of them repeated, tags with and without a
post before it, a restart with a resume, a reset and the whole again -- on 100 pairs of bwa_path_v1.npz in two barcodes of 50.

Every array a call hands out is compared byte for byte with what the same call handed out the first time: a phase that rewinds the arena to
the wrong mark, or reads memory a rewind gave away, changes them (the host double fills released memory with 0xDD and frees it; fresh memory
is 0xAB).  On the double the bytes live in the arena after each phase are compared with those after the same phase in the first cycle,
which pins both that nothing grows from cycle to cycle and that each phase rewinds to its own mark; a reset leaves none."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import workloads
from arachne_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "hostsim", "libarx_hostsim.so")
N_READS = 200
PO, FLAGS = [0, 50, 100], [True, True]


class Driver:
    def __init__(self, ref, seqs, lens, count_live):
        self.ref, self.seqs, self.lens = ref, seqs, lens
        self.b = ref.batch(seqs, lens)
        self.first = {}   # call -> the bytes of every array of its first result
        self.live = {}    # phase -> bytes live in the arena after it, first cycle
        self.count_live = count_live
        if count_live:
            ref.lib.arx_test_arena_live_bytes.restype = C.c_int64
            ref.lib.arx_test_arena_live_bytes.argtypes = [C.c_void_p]

    def same(self, call, arrays):
        got = {k: np.ascontiguousarray(v).tobytes() for k, v in arrays.items() if isinstance(v, np.ndarray)}
        want = self.first.setdefault(call, got)
        for k in want:
            assert got[k] == want[k], (call, k)

    def live_is(self, phase, expect=None):
        """the arena holds what it held after this phase in the first cycle (or `expect` bytes); -> the bytes"""
        if not self.count_live:
            return 0
        n = int(self.ref.lib.arx_test_arena_live_bytes(self.b.h))
        assert n == (self.live.setdefault(phase, n) if expect is None else expect), (phase, n, self.live, expect)
        return n

    def refused(self, fn, *args, match):
        with pytest.raises(api.ArachneError, match=match):
            self.ref._check(fn(self.ref.h, self.b.h, *args))

    def run(self):
        self.same("fetch", self.b.run().fetch())
        self.live_is("run")

    def rfa(self):
        self.same("rfa", self.b.rfa(PO, FLAGS))
        self.live_is("rfa")

    def post(self):
        self.same("post", self.b.post())
        self.live_is("post")

    def tags(self, phase="tags"):
        self.same("tags", dict(tags=self.b.tags()))
        return self.live_is(phase)

    def tags_then_post(self):
        """behind rfa(): tags without post lie right behind placement, and a later post takes their place"""
        lib, none = self.ref.lib, None
        if self.count_live:
            self.tags("tags_only")
            self.live_is("tags_only", self.live["rfa"] + self.live["tags"] - self.live["post"])
        else:
            self.tags()
        self.refused(lib.arx_batch_post_fetch, none, none, none, none, match="before arx_batch_post")
        self.post()
        self.refused(lib.arx_batch_tags_fetch, none, match="before arx_batch_tags")
        self.tags()

    def cycle(self):
        lib, none = self.ref.lib, None
        self.run(); self.rfa(); self.post(); self.tags()
        self.post()                                      # post again: the tags are gone
        self.refused(lib.arx_batch_tags_fetch, none, match="before arx_batch_tags")
        self.tags()
        self.rfa()                                       # rfa again, in the memory of the first: post and tags are gone
        self.refused(lib.arx_batch_post_fetch, none, none, none, none, match="before arx_batch_post")
        self.refused(lib.arx_batch_tags_fetch, none, match="before arx_batch_tags")
        self.post(); self.tags()
        self.rfa()
        self.tags_then_post()
        self.b.run(api.STAGE_SEED)                       # a stage asked for again restarts the batch ...
        self.live_is("seed")
        self.refused(lib.arx_batch_rfa_fetch, none, none, match="before arx_batch_rfa")
        self.refused(lib.arx_batch_fetch, none, none, none, none, match="before arx_batch_run")
        self.run()                                       # ... and run(ALN) resumes behind the seeds; placement stays discarded
        self.refused(lib.arx_batch_rfa_fetch, none, none, match="before arx_batch_rfa")
        self.refused(lib.arx_batch_post, none, match="before arx_batch_rfa")


def _drive(lib_path, count_live):
    z = np.load(os.path.join(HERE, "golden", "bwa_path_v1.npz"))
    prefix = workloads.unpack_index(z, tempfile.mkdtemp(prefix="arx_arena_"))
    seqs, lens = z["reads"][:N_READS], z["lens"][:N_READS]
    ref = api.Reference(prefix, lib_path=lib_path)
    try:
        d = Driver(ref, seqs, lens, count_live)
        d.live_is("created", 0)
        d.cycle()
        d.b.reset(seqs, lens)                            # free_work: the whole arena is handed back
        d.live_is("reset", 0)
        d.cycle()
        if count_live:
            assert 0 < d.live["seed"] < d.live["run"] < d.live["rfa"] < d.live["post"] < d.live["tags"]
        d.b.free()
        e = Driver(ref, seqs, lens, count_live)          # a handle whose first call behind placement is tags: post has no mark of its own yet
        e.first, e.live = d.first, d.live
        e.run(); e.rfa(); e.tags_then_post()
        e.b.free()
    finally:
        ref.close()


def test_arena_lifecycle_hostsim(built):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SIM)])
    _drive(SIM, True)


@pytest.mark.gpu
def test_arena_lifecycle_gpu(built):
    _drive(api.LIB_PATH, False)

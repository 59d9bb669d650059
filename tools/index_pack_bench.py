#!/usr/bin/env python3
"""The index build with the FASTA packed on the host (arx_index_build, the yardstick) beside the build that reads and packs it on the GPU
(arx_index_build_ex), in one process on the same files.

One seeded genome from arachne_amd/synth.py (make_genome(fast=True), 24 contigs in the proportions of bench.py's GRCh38-size recipe, --bases in
all: the default is that recipe's size) as plain text, as ordinary gzip and as BGZF (blocks of 65,280 bytes), both at level 1, files in the
page cache.  One JSON line per measurement:
  input     the sizes
  build     arm "host" (plain text only: it reads nothing else) or "device", form plain / gzip / bgzf, the call's seconds, its phases (host:
            arx_index_build_times; device: the call's stats) and whether its five files have the digests of the first host build
--passes times per arm and form, alternating.  Before any time is reported the five files of the pass are compared by digest.
  summary   per arm and form the minimum and the range (max - min) of the seconds
Usage: index_pack_bench.py [--bases N] [--passes 3] [--out-dir DIR] [--pack-only]"""
import argparse
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bgzfio  # noqa: E402  (tests/bgzfio.py: the BGZF writer)
from arachne_amd import api, synth  # noqa: E402

GRCH38_LENS = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422, 135086622, 133275309,
               114364328, 107043718, 101991189, 90338345, 83257441, 80373285, 58617616, 64444167, 46709983, 50818468, 156040895, 57227415]   # bench.py's recipe
EXTS = ("bwt", "sa", "pac", "ann", "amb")


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        while True:
            b = f.read(1 << 24)
            if not b:
                return h.hexdigest()
            h.update(b)


def write_forms(plain, gz, bgzf):
    """the plain file again as gzip (one member) and as BGZF, piece by piece"""
    c = zlib.compressobj(1, zlib.DEFLATED, 31)
    with open(plain, "rb") as f, open(gz, "wb") as g, open(bgzf, "wb") as b:
        while True:
            t = f.read(256 * bgzfio.BLOCK_IN)
            if not t:
                break
            g.write(c.compress(t))
            b.write(bgzfio.write_bgzf(t, level=1, eof=False))
        g.write(c.flush())
        b.write(bgzfio.EOF_BLOCK)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=sum(GRCH38_LENS))
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--pack-only", action="store_true", help="the device arm stops behind .pac/.ann/.amb (only those three are compared)")
    args = ap.parse_args()
    d = args.out_dir or tempfile.mkdtemp(prefix="arx_index_pack_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(d, exist_ok=True)
    scale = args.bases / sum(GRCH38_LENS)
    lens = [max(1000, int(x * scale)) for x in GRCH38_LENS]
    g = synth.make_genome(20250905 + 3, lens, fast=True)
    plain, gz, bgzf = os.path.join(d, "g.fa"), os.path.join(d, "g.fa.gz"), os.path.join(d, "g.bgzf.fa.gz")
    g.write_fasta(plain)
    del g
    write_forms(plain, gz, bgzf)
    forms = dict(plain=plain, gzip=gz, bgzf=bgzf)
    for p in forms.values():                                     # into the page cache
        with open(p, "rb") as f:
            while f.read(1 << 24):
                pass
    print(json.dumps(dict(what="input", bases=sum(lens), contigs=len(lens), **{k + "_bytes": os.path.getsize(p) for k, p in forms.items()})), flush=True)
    want, series = None, {}
    arms = [("host", "plain")] + [("device", k) for k in forms]
    for rep in range(args.passes):
        for arm, form in arms:
            prefix = os.path.join(d, "%s_%s" % (arm, form))
            exts = EXTS if arm == "host" or not args.pack_only else ("pac", "ann", "amb")
            for e in EXTS:
                if os.path.exists(prefix + "." + e):
                    os.remove(prefix + "." + e)
            t = time.time()
            if arm == "host":
                api.index_build(forms[form], prefix)
                phases = {k[:-2] + "_ms": round(v * 1e3, 1) for k, v in api.index_build_times().items()}
            else:
                st = api.index_build(forms[form], prefix, pack="device", pack_only=args.pack_only)
                phases = {k[:-3] + "_ms": round(v / 1e3, 1) for k, v in st.items() if k.endswith("_us")}
                phases.update(windows=st["windows"], holes=st["holes"], ambiguous=st["ambiguous"])
            s = time.time() - t
            digests = {e: sha(prefix + "." + e) for e in exts}
            if want is None:
                want = digests                                   # the first host build
            same = all(digests[e] == want[e] for e in exts)
            print(json.dumps(dict(what="build", arm=arm, form=form, rep=rep, files_are_the_host_builders=same, seconds=round(s, 3), **phases)), flush=True)
            if not same:
                print(json.dumps(dict(what="error", text="the files of %s / %s differ from the host builder's: no time is reported" % (arm, form))), flush=True)
                return 1
            series.setdefault(arm + "/" + form, []).append(round(s, 3))
    print(json.dumps(dict(what="summary", **{k: dict(min_s=min(v), range_s=round(max(v) - min(v), 3), all_s=v) for k, v in series.items()})), flush=True)
    if not args.out_dir:
        shutil.rmtree(d, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

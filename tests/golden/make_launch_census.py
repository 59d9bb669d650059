"""Records tests/golden/launch_census_v1.json: per case of tests/test_launch_paths_gpu.py, launch name -> [calls, items] of kernel_times().

Run on the GPU from a tree whose library is built from the commit BEFORE the one launch path (csrc/hip_launch.h), with this file and
tests/test_launch_paths_gpu.py copied into that tree -- the table is what the hand-written launches did:

    python tests/golden/make_launch_census.py record OUT.json      (once per recording, each in a process of its own)
    python tests/golden/make_launch_census.py merge A.json B.json  (writes the table if the two recordings agree)

Every case must also pass the parity checks of the test while it is recorded.  merge refuses a table whose calls differ anywhere or whose
items differ in more than two fields; an items field that differs is written as null (not compared by the test) and printed.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (os.path.dirname(TESTS), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)


def record(out):
    import subprocess
    import oradrv
    import parity
    import rfadrv
    import test_launch_paths_gpu as t
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(TESTS), "oracle"), "oracle"])
    fa, rs = t.make_workload()
    po = rs.pair_offsets()
    flags = [rfadrv.worth_running_rfa(rs.barcodes[i], int(po[i + 1] - po[i])) for i in range(len(po) - 1)]
    ora = oradrv.Oracle(fa).batch(rs.seqs, rs.lens, n_threads=8)
    cases = {}
    for var in t.CASES:
        os.environ.pop("ARX_TEXT_INDEX", None)
        if "ARX_TEXT_INDEX" in var:
            os.environ["ARX_TEXT_INDEX"] = str(var["ARX_TEXT_INDEX"])
        ref = t.api.load_reference(fa, 0)
        try:
            t.set_case_env(var, os.environ.__setitem__, lambda k: os.environ.pop(k, None))
            dev, cands, census = t.run_case(ref, rs, flags)
            parity.check_final(dev, ora)
            names, offs, clens, alt, l_pac = ref.contigs()
            parity.check_rfa(cands, rfadrv.oracle_rfa(ora, rs.lens, po, flags, l_pac, offs))
        finally:
            ref.close()
        cases[t.label(var)] = census
        print(f"{t.label(var):32s} {len(census)} launch names, {sum(c for c, _ in census.values())} calls", flush=True)
    with open(out, "w") as f:
        json.dump({"cases": cases}, f, indent=0, sort_keys=True)


def merge(a, b):
    with open(a) as f:
        ca = json.load(f)["cases"]
    with open(b) as f:
        cb = json.load(f)["cases"]
    assert sorted(ca) == sorted(cb)
    left_out = []
    for case in ca:
        assert sorted(ca[case]) == sorted(cb[case]), case
        for name in ca[case]:
            assert ca[case][name][0] == cb[case][name][0], ("calls differ", case, name, ca[case][name], cb[case][name])
            if ca[case][name][1] != cb[case][name][1]:
                left_out.append((case, name, ca[case][name][1], cb[case][name][1]))
                ca[case][name][1] = None
    print(f"items fields left out: {left_out}")
    assert len(left_out) <= 2, "more than two items fields differ between the recordings"
    out = os.path.join(HERE, "launch_census_v1.json")
    with open(out, "w") as f:
        f.write("{\"cases\": {\n" + ",\n".join(f" {json.dumps(c)}: {json.dumps(ca[c], sort_keys=True)}" for c in sorted(ca)) + "\n}}\n")
    print(f"wrote {out}: {len(ca)} cases")


if __name__ == "__main__":
    if sys.argv[1] == "record":
        record(sys.argv[2])
    else:
        merge(sys.argv[2], sys.argv[3])

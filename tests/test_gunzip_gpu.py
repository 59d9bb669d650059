"""GPU test of the chunked gzip inflate (arachne_amd/csrc/dev_gunzip.h, hip_gunzip.h, gunzip_host.h) through arx_selftest_gunzip: every case of
gunzipcases.py on the device.  The bytes are compared with Python's zlib, member by member, under gzread's rule for what follows a member; the
return value and the statistics with what the case states; and the counts that do not depend on scheduling -- members, chunks, candidates,
accepted chunks, refuted candidates, DEFLATE blocks, and why the host took over -- with the host twin's for the same sizes."""
import pytest

import gunzipcases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from arachne_amd import api as a
    return a


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """every case through the host twin, built plain (the sanitizers are the CPU test's, test_gunzip_sim.py): run once, shared"""
    sim = gc.build_sim(str(tmp_path_factory.mktemp("gunzipsim")), sanitize=False)
    tmp = str(tmp_path_factory.mktemp("gunzip_runs"))
    return {name: gc.run_sim(sim, tmp, case) for name, case in gc.cases().items()}


def on_device(api, case):
    want = gc.expected(case.data)
    return api.selftest_gunzip(case.data, case.chunk, case.slab, case.expand, cap=(len(want[0]) if want else 0) + 64)


@pytest.mark.parametrize("name", sorted(gc.cases()))
def test_case(api, twin, name):
    case = gc.cases()[name]
    res = on_device(api, case)
    gc.check(case, res, name)
    if res["rc"] == gc.ARX_OK:
        assert {k: res[k] for k in gc.STABLE} == {k: twin[name][k] for k in gc.STABLE}, name
        assert res["markers"] == twin[name]["markers"] and res["launches"] == twin[name]["launches"] and res["host_bytes"] == twin[name]["host_bytes"], name


def test_sizes_outside_their_bounds_are_refused(api):
    case = gc.cases()["level6_chunk4096"]
    for chunk, slab, expand in ((63, 4096, 16), (4096, 8191, 16), (4096, 1 << 28, 16), (4096, 65536, 1033), (4096, 1 << 27, 16), (-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        assert api.selftest_gunzip(case.data, chunk, slab, expand, cap=400000)["rc"] == gc.ARX_E_ARG, (chunk, slab, expand)
    assert api.selftest_gunzip(case.data, case.chunk, case.slab, case.expand, cap=len(gc.expected(case.data)[0]) - 1)["rc"] == gc.ARX_E_ARG
    assert api.selftest_gunzip(b"", cap=16) == dict(api.selftest_gunzip(b"", cap=16), rc=0, out=b"", members=0, launches=0)


def test_the_defaults_read_a_file(api):
    case = gc.cases()["level6_chunk4096"]
    want = gc.expected(case.data)[0]
    res = api.selftest_gunzip(case.data, cap=len(want))
    assert res["rc"] == 0 and res["out"] == want and res["fallback"] == 0 and res["host_bytes"] == 0 and res["launches"] == 1


def test_no_gzip_file_comes_back_as_it_is(api):
    data = b"@r1\nACGT\n+\nIIII\n" * 50
    res = api.selftest_gunzip(data, cap=len(data))
    assert res["rc"] == 0 and res["out"] == data and res["members"] == 0 and res["launches"] == 0

"""The device inflate on the GPU (arx_selftest_inflate; arachne_amd/csrc/dev_inflate.h, hip_inflate.h): the block cases of inflatecases.py,
the ones test_inflate_sim.py runs under the sanitizer on the host, through the kernel.  Bit-exact against Python's zlib; statuses, the count
of bytes in front of the first bad block, the entry's return value and its stats against what the test parsed."""
import pytest

import bgzfcases
import bgzfio
import inflatecases as ic
from arachne_amd import api

pytestmark = pytest.mark.gpu


def _check(name, case):
    r = api.selftest_inflate(case.chain, fill=0xA5)
    assert r["rc"] == case.ret, (name, r["rc"], r["status"])
    assert r["status"] == case.status, (name, r["status"])
    offs = ic.block_offsets(case.chain)
    assert (r["blocks"], r["compressed_bytes"], r["inflated_bytes"]) == (len(offs), len(case.chain), sum(n for _, n in offs)), name
    first_bad = next((k for k, s in enumerate(case.status) if s != ic.OK), len(offs))
    assert r["out_len"] == sum(n for _, n in offs[:first_bad]), name
    for (o, n), data, st in zip(offs, case.data, case.status):
        if st == ic.OK:
            assert r["out"][o:o + n] == data, name
        else:
            assert r["out"][o:o + n] == b"\xa5" * n, name           # a bad block writes nothing
    if case.n_deflate is not None:
        assert r["deflate_blocks"] == case.n_deflate, name


@pytest.mark.parametrize("name", sorted(ic.good_cases()))
def test_good_blocks(name):
    _check(name, ic.good_cases()[name])


@pytest.mark.parametrize("name", sorted(ic.damage_cases()))
def test_damaged_block_among_good_neighbours(name):
    _check(name, ic.damage_cases()[name])


def test_chains_that_do_not_tile_are_refused():
    for name, chain in ic.untiled_chains().items():
        assert api.selftest_inflate(chain)["rc"] == ic.ARX_E_ARG, name
    assert api.selftest_inflate(b"")["rc"] == 0


def test_round_trip_through_the_device_deflate():
    """arx_selftest_bgzf's output for every input of bgzfcases.py inflates to the input"""
    for name, data in bgzfcases.edge_inputs().items():
        raw, forms = api.bgzf_selftest(data)
        r = api.selftest_inflate(raw)
        assert r["rc"] == 0 and r["out"] == data and r["blocks"] == forms["blocks"], name
        assert r["deflate_blocks"] == forms["blocks"]               # the device deflate writes one DEFLATE block a BGZF block

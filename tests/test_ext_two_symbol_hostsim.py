"""The two-symbol form of an extension's arithmetic (dev_fm.h ext_finish<true>, what k_seed_bwd_g<true> runs) against extend1(), on the CPU.

ext_finish<true> counts symbol c and one more symbol at each end of the interval and takes the position of child c on the other strand from
s_0 + s_1 + s_2 + s_3 = ik.s - cond (the identity is written beside the function); extend1() counts all four symbols.  The same header compiles
for the host, so tests/hostsim/ext_two_symbol.cpp -- a program of its own, built here with the address and undefined-behaviour sanitizers --
calls the very functions the kernel calls: on the Occ blocks of a random text with its reverse complement (naive suffix sort, primary row
inside) it visits every bi-interval within 8 extensions of the empty string in either direction and compares all four fields of every child,
both directions, c = 0..3, and the identity itself.  The program fails if it did not meet an interval that contains the primary row, the row -1,
an interval of one row, rows at block offsets 0 and 127 and at quarter offsets 31 and 32, or both ends in one block and in two."""
import os
import re
import subprocess
import tempfile

import pytest

HOSTSIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")


@pytest.fixture(scope="module")
def program():
    exe = os.path.join(tempfile.mkdtemp(prefix="arx_ext_two_symbol_"), "ext_two_symbol")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(HOSTSIM, "ext_two_symbol.cpp")])
    return exe


@pytest.mark.parametrize("half,seed", [(1500, 0), (1987, 1)])   # 3,000 symbols (23.4 blocks) and 3,974 (31.05: the last block nearly empty)
def test_two_symbol_extension_equals_extend1(program, half, seed):
    r = subprocess.run([program, str(half), str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    got = dict((k, int(v)) for k, v in re.findall(r"(\w+) (\d+)", r.stdout))
    # (the program itself refuses to pass without its edges; these are the same facts read from its report)
    assert got["extensions"] >= 8 * (1 + 4 + 16 + 64 + 256 + 1024), r.stdout   # at least every string of up to five symbols: a text of thousands holds them all
    assert got["with_primary"] > 0 and got["row_minus1"] > 0 and got["s1"] > 0, r.stdout
    assert got["one_block"] > 0 and got["two_blocks"] > 0 and got["off0"] and got["off31"] and got["off32"] and got["off127"], r.stdout

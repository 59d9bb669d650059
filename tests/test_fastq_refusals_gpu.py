"""The refusals of the four FASTQ file-pair calls, code and full text (arx_fastq_sort, arx_fastq_sort_ex, arx_fastq_standardize,
arx_fastq_prepare): the neighbouring tests hold the codes and a few substrings, this one every message byte for byte, against
tests/golden/fastq_refusals.json -- recorded by fqrefusalcases.py from the commit before the calls' host plumbing became one path, so a
changed sentence, a lost remedy or another order of the checks shows here.  Out-of-memory texts are not provoked.
And the one correction that came with the one path: a call never removes a file it did not create."""
import json

import pytest

import fqrefusalcases as rc
from arachne_amd import api

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(rc.GOLDEN))
IDS = [(call, case) for call in rc.CALLS for case in sorted(GOLDEN[call])]


@pytest.fixture(scope="module")
def refusals(tmp_path_factory):
    return rc.run(str(tmp_path_factory.mktemp("refusals")))


def test_every_call_is_asked_what_the_record_holds(refusals):
    got, _ = refusals
    assert sorted(GOLDEN) == sorted(rc.CALLS) and {c: sorted(v) for c, v in got.items()} == {c: sorted(v) for c, v in GOLDEN.items()}
    for call in rc.CALLS:                                                  # what the issue of the one path lists, per call
        want = {"unknown_flag", "null_output", "same_output_twice", "output_is_an_input", "missing_input", "output_under_a_file", "flipped_crc"}
        want |= {"bad_format", "undetectable"} if call in rc.HAS_FORMAT else set()
        want |= {"run_bytes_minus_two", "run_bytes_under_the_window", "tmp_dir_under_a_file", "record_longer_than_a_run"} if call in rc.HAS_RUNS else set()
        want |= {"max_bytes_one_short"} if call in rc.HAS_MAX else set()
        assert want <= set(GOLDEN[call]), call


@pytest.mark.parametrize("call,case", IDS, ids=["%s-%s" % i for i in IDS])
def test_code_and_text(refusals, call, case):
    got, want = refusals[0][call][case], GOLDEN[call][case]
    print(call, case, got)
    assert got["code"] == want["code"] and got["msg"] == want["msg"]


def test_a_tmp_name_the_call_did_not_create_is_not_removed(refusals):
    got, kept = refusals
    for call in rc.CALLS:
        assert got[call]["tmp_name_is_a_directory"]["code"] == api.ARX_E_IO, call
        assert kept[call], call                                            # <out>/o1.fq.tmp, a directory made before the call, is still there

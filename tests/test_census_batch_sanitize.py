"""Host sanitizer coverage of the host side of mg_census_batch (DESIGN.md
§3.17): mythril_amd/csrc/mg_census_batch.h — the check of a job's counts
(mg_census_shape_ok), the blocks rule and the plan of the batch's device
buffer with its chunk rule (mg_census_batch_plan), the code the C ABI runs
before it uploads anything — built with g++ -fsanitize=address,undefined into
the stand-alone tests/fuzz_census_batch.cpp and driven with valid, mutated and
random shapes.  CPU only; nothing is loaded into Python."""

import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fuzz_binary(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("fuzz") / "fuzz_census_batch")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mythril_amd", "csrc"),
           os.path.join(ROOT, "tests", "fuzz_census_batch.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    return out


def test_shape_check_blocks_and_plan_under_asan_ubsan(fuzz_binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_binary, "3000"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    n = stats["iterations"]
    # valid shapes pass the check, and every batch of them is planned
    assert stats["valid_accepted"] == n == stats["valid_planned"]
    # a mutated count is caught often; the plan holds for any counts whose
    # probe regions fit, which most mutations leave alone
    assert 0 < stats["mutated_accepted"] < stats["mutated"]
    assert stats["mutated_planned"] > stats["mutated"] // 2
    # three random words are a valid shape now and then, a batch of them rarely
    assert stats["random_accepted"] < n // 4
    assert 0 < stats["random_planned"] < n
    # shared arguments out of range: three cases in four
    assert n // 2 < stats["shared_refused"] < n
    assert stats["blocks_checked"] == n
    # every kind of refusal was met, and accepted plans were laid out in a
    # buffer of exactly their size
    assert stats["refused_chunk_bytes"] > 0 and stats["refused_no_fit"] > 0
    assert stats["refused_overflow"] > 0
    assert stats["laid_out"] > n and stats["bytes_laid"] > 0

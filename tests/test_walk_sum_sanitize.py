"""Host sanitizer coverage of the safety boundary of the aims through sums
(DESIGN.md §3.15): mythril_amd/csrc/mg_walk_sum.h — the validator
mg_walk_sum_ok and the lane function mg_walk_sum_lane (apart and in place),
the code the kernels run — built with g++ -fsanitize=address,undefined into
the stand-alone tests/fuzz_walk_sum.cpp and driven with valid, mutated and
random tables.  CPU only; nothing is loaded into Python."""

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
    out = str(tmp_path_factory.mktemp("fuzz") / "fuzz_walk_sum")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mythril_amd", "csrc"),
           os.path.join(ROOT, "tests", "fuzz_walk_sum.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    return out


def test_validator_and_lane_function_under_asan_ubsan(fuzz_binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_binary, "3000"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    assert stats["valid_accepted"] == stats["iterations"]
    # mutations are caught often, and accepted ones still move in bounds;
    # random words essentially never pass
    assert 0 < stats["mutated_accepted"] < stats["mutated"]
    assert stats["random_accepted"] < stats["iterations"] // 20
    assert stats["aimed_lanes"] > stats["iterations"]
    # slots do resolve to leaves, so slot pieces are scattered and gathered
    assert stats["resolved_slots"] > stats["iterations"]
    # and linear entries were applied, in every mode
    assert stats["linear_lanes"] > stats["iterations"]

"""Host sanitizer coverage of the host side of mg_carry_batch (DESIGN.md
§3.18): mythril_amd/csrc/mg_carry.h — the checks of the shared counts and of a
leaf table, the plan of the batch's device buffer (mg_carry_plan) and the fill
kernel's lane function (mg_carry_fill_lane) writing into a buffer of exactly
the planned size under random pin masks — built with g++
-fsanitize=address,undefined into the stand-alone tests/fuzz_carry.cpp and
driven with valid, mutated and random shapes.  CPU only; nothing is loaded into
Python."""

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
    out = str(tmp_path_factory.mktemp("fuzz") / "fuzz_carry")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mythril_amd", "csrc"),
           os.path.join(ROOT, "tests", "fuzz_carry.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    return out


def test_plan_and_fill_under_asan_ubsan(fuzz_binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_binary, "1000"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    n = stats["iterations"]
    # every valid batch is planned; the plan holds for any counts short of 2^64
    # bytes, which random words at 256 jobs sometimes exceed
    assert stats["valid_planned"] == n
    assert stats["mutated_planned"] > stats["mutated"] // 2
    assert 0 < stats["random_planned"] <= n
    # shared arguments out of range: four cases in five; every bad leaf table
    assert n // 2 < stats["shared_refused"] < n
    assert stats["gen_refused"] == n and stats["overflow_refused"] > 0
    # accepted plans were laid out in a buffer of exactly their size and filled
    # there: pinned and generated leaves, every class of the generator
    assert stats["laid_out"] >= n and stats["bytes_laid"] > 0
    assert stats["pinned"] > 0 and stats["generated"] > 0
    assert stats["pinned"] + stats["generated"] == stats["lanes_filled"]
    assert all(c > 0 for c in stats["classes"])

"""Host sanitizer coverage of the host side of mg_carry_census (DESIGN.md
§3.20): mythril_amd/csrc/mg_carry.h — the plan of its device buffer
(mg_carry_census_plan) and the start rule (mg_carry_pick_starts) reading counter
blocks and writing starts inside a buffer of exactly the planned size — built
with g++ -fsanitize=address,undefined into the stand-alone
tests/fuzz_carry_census.cpp.  CPU only; nothing is loaded into Python."""

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
    out = str(tmp_path_factory.mktemp("fuzz") / "fuzz_carry_census")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mythril_amd", "csrc"),
           os.path.join(ROOT, "tests", "fuzz_carry_census.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    return out


def test_census_plan_and_start_rule_under_asan_ubsan(fuzz_binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_binary, "300"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    n = stats["iterations"]
    assert stats["valid_planned"] == n
    assert stats["walkers_refused"] == stats["roots_refused"] == stats["mask_refused"] == \
        stats["ladder_refused"] == n
    assert stats["overflow_refused"] > 0
    # accepted plans were laid out in a buffer of exactly their size; there the
    # rule ran on random words and on blocks counted from verdict bits, where it
    # equalled the list built from the bits and no column came twice
    assert stats["laid_out"] > n // 2 and stats["bytes_laid"] > 0
    assert stats["jobs_picked"] == stats["random_picked"] > n
    # every situation: a list shorter than W, longer than W, a hit, sole columns as starts
    for key in ("padded", "longer", "hits", "sole_starts", "distinct_checked"):
        assert stats[key] > 0, key

"""Host sanitizer coverage of the host side of mg_carry_ladder_sets (DESIGN.md
§3.21): mythril_amd/csrc/mg_carry.h — the checks of the counts and of a job's
rung_set, the plan of the device buffer (mg_carry_sets_plan) and the set fill
kernel's lane function (mg_carry_fill_set_lane) writing into a buffer of exactly
the planned size under random rung counts, set counts, masks and rung_sets —
built with g++ -fsanitize=address,undefined into the stand-alone
tests/fuzz_carry_sets.cpp.  CPU only; nothing is loaded into Python."""

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
    out = str(tmp_path_factory.mktemp("fuzz") / "fuzz_carry_sets")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mythril_amd", "csrc"),
           os.path.join(ROOT, "tests", "fuzz_carry_sets.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    return out


def test_sets_plan_and_set_fill_under_asan_ubsan(fuzz_binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_binary, "400"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    n = stats["iterations"]
    assert stats["valid_planned"] == n
    # n_sets of 0 and 9, a rung_set entry at or above n_sets (and a null one), R x lanes above
    # 2^20 (and exactly 2^20 accepted), the shared counts of the ladder, sizes beyond 64 bits
    assert stats["sets_refused"] == stats["rung_set_refused"] == stats["cols_refused"] == \
        stats["shared_refused"] == n
    assert stats["overflow_refused"] > 0
    # accepted plans were laid out in a buffer of exactly their size and filled there, every
    # column held to its rung's mask and to the rows of its rung's set: every set of the eight,
    # and the repeated last rung of jobs with fewer rungs than their batch
    assert stats["laid_out"] >= n and stats["bytes_laid"] > 0
    assert stats["pinned"] > 0 and stats["generated"] > 0
    assert stats["pinned"] + stats["generated"] == stats["cols_filled"]
    assert all(c > 0 for c in stats["set_cols"]) and len(stats["set_cols"]) == 8
    assert sum(stats["set_cols"]) == stats["cols_filled"] and stats["surplus"] > 0

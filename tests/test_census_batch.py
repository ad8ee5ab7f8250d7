"""The host side of mg_census_batch (csrc/mg_census_batch.h)
without a GPU: the exports, the plan of the batch's device buffer, its
refusals, the chunk rule and the blocks rule."""

import ctypes as C

import numpy as np
import pytest

from mythril_amd import engine as E
from mythril_amd.engine import CensusShape, EngineError

MAX_PROBE_BYTES = 256 << 20          # csrc/mg_census.h
PDESC_BYTES = 72                     # sizeof(mg_pdesc), csrc/mg_device.h


def test_library_exports_the_entries():
    lib = E.load_library(check_digest=False)
    for name in ("mg_census_batch", "mg_batch_witness", "mg_census_batch_plan_host",
                 "mg_census_batch_blocks_host"):
        assert name in E.EXPORTS and hasattr(lib, name)
    assert E.CENSUS_BATCH_MAX_JOBS == E.WALK_BATCH_MAX_JOBS == 256


def words(r):
    return 5 * r + 2                 # mg_census_words


def up(b):
    return (b + 255) & ~255


@pytest.mark.parametrize("shapes, n_cand, chunk", [
    ([(1, 3, 0)], 1000, 0),
    ([(1, 3, 0), (2, 257, 0), (5, 33, 2)], 1000, 256),
    ([(2, 1024, 0), (1, 1, 0)], 1, 0),
    ([(7, 65, 6)] * 5, 1 << 16, 512),
    ([(1, 31, 0), (4, 1024, 0)], 0, 0),
])
def test_plan_tiles_the_buffer(shapes, n_cand, chunk):
    ss = [CensusShape(*s) for s in shapes]
    offs, total, got = E.census_batch_plan_host(ss, n_cand, chunk)
    n = len(ss)
    assert len(offs) == E.CENSUS_BATCH_SHARED + n * E.CENSUS_BATCH_JOB_REGIONS
    assert got == (chunk or 1 << 16)
    lanes = min(n_cand, got)
    count_b = up(words(max(s[1] for s in shapes)) * 8)
    probe_b = up(max(s[0] for s in shapes) * 8 * lanes * 4)
    # address order: descriptors, records, every counter block, every probe region
    order = [int(offs[0]), int(offs[1])] + [int(offs[2 + 2 * g]) for g in range(n)] + \
            [int(offs[3 + 2 * g]) for g in range(n)]
    assert order[0] == 0 and order == sorted(order)
    assert all(o % 256 == 0 for o in order) and total % 256 == 0
    ends = order[1:] + [total]
    sizes = [e - o for o, e in zip(order, ends)]
    assert sizes[0] >= n * PDESC_BYTES and sizes[1] >= n * 24          # two pointers, a count
    assert sizes[2:2 + n] == [count_b] * n                              # the common stride
    assert sizes[2 + n:] == [probe_b] * n
    # every job's own counter block and rows lie inside its regions
    for (n_probes, n_roots, m0) in shapes:
        assert words(n_roots) * 8 <= count_b
        assert (m0 + (n_roots + 255) // 256) * 8 * lanes * 4 <= probe_b
    assert total == order[-1] + probe_b


def test_plan_refusals():
    one = [CensusShape(1, 3, 0)]
    with pytest.raises(EngineError, match=r"census_batch: 0 jobs outside 1\.\.256"):
        E.census_batch_plan_host([], 1000)
    with pytest.raises(EngineError, match=r"census_batch: 257 jobs outside 1\.\.256"):
        E.census_batch_plan_host(one * 257, 1000)
    for chunk in (100, 255, 257, 384 + 64):
        with pytest.raises(EngineError, match="census_batch: chunk %d is not a multiple of 256"
                           % chunk):
            E.census_batch_plan_host(one, 1000, chunk)
    # a chunk past the byte cap: 16 jobs x 2 probes x 32 bytes per candidate
    ss = [CensusShape(2, 3, 0)] * 16
    fit = MAX_PROBE_BYTES // (16 * 2 * 32)
    assert fit % 256 == 0
    assert E.census_batch_plan_host(ss, 1 << 20, fit)[2] == fit
    need = 16 * 2 * 32 * (fit + 256)
    with pytest.raises(EngineError, match=r"census_batch: %d bytes needed .* at chunk %d"
                       % (need, fit + 256)):
        E.census_batch_plan_host(ss, 1 << 20, fit + 256)
    # 256 lanes do not fit: the census view wording of mg_census
    big = [CensusShape(200, 3, 0)] * 256
    assert 256 * 200 * 32 * 256 > MAX_PROBE_BYTES
    with pytest.raises(EngineError, match=r"census_batch: .*load the census view"):
        E.census_batch_plan_host(big, 1000)
    with pytest.raises(EngineError, match=r"census_batch: .*bytes needed"):
        E.census_batch_plan_host(big, 1000, 256)
    # overflowing counts
    huge = [CensusShape(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)] * 256
    with pytest.raises(EngineError, match="census_batch: .*(64 bits|bytes needed)"):
        E.census_batch_plan_host(huge, 1 << 62, 1 << 62)
    with pytest.raises(EngineError, match="census_batch: .*64 bits"):
        E.census_batch_plan_host(huge, 1 << 62, (1 << 64) - 256)
    with pytest.raises(EngineError, match="census_batch: .*census view"):
        E.census_batch_plan_host(huge, 1 << 62, 0)
    # null pointers through the raw entry
    lib = E.load_library(check_digest=False)
    arr = (CensusShape * 1)(*one)
    offs = np.zeros(4, dtype=np.uint64)
    t, c = C.c_uint64(), C.c_uint64()
    p = offs.ctypes.data_as(C.c_void_p)
    why = C.create_string_buffer(64)
    assert lib.mg_census_batch_plan_host(arr, 1, 10, 0, p, C.byref(t), C.byref(c), why, 64) == 0
    assert why.value == b""
    assert lib.mg_census_batch_plan_host(None, 1, 10, 0, p, C.byref(t), C.byref(c), why, 64) == -1
    assert why.value == b"null argument"
    assert lib.mg_census_batch_plan_host(arr, 1, 10, 0, None, C.byref(t), C.byref(c), None, 0) == -1
    assert lib.mg_census_batch_plan_host(arr, 1, 10, 0, p, None, C.byref(c), None, 0) == -1
    assert lib.mg_census_batch_plan_host(arr, 1, 10, 0, p, C.byref(t), None, None, 0) == -1


def test_chunk_zero_is_the_largest_multiple_of_256_that_fits():
    plan = lambda shapes, n=1 << 20: E.census_batch_plan_host([CensusShape(*s) for s in shapes],
                                                              n, 0)[2]
    assert plan([(1, 3, 0)]) == 1 << 16                              # MG_CENSUS_CHUNK
    assert plan([(2, 3, 0)] * 16) == 1 << 16                         # 64 MiB
    assert plan([(1, 3, 0)] * 128) == 1 << 16                        # exactly 256 MiB
    assert plan([(1, 3, 0)] * 256) == 1 << 15
    assert plan([(1, 3, 0)] * 255 + [(3, 3, 0)]) == (MAX_PROBE_BYTES // (256 * 3 * 32)) // 256 * 256
    assert plan([(3, 3, 0)] * 100) == 27904 and 27904 % 256 == 0
    assert 100 * 3 * 32 * 27904 <= MAX_PROBE_BYTES < 100 * 3 * 32 * (27904 + 256)
    assert plan([(128, 3, 0)] * 256) == 256                          # the last that fits
    # and the split by which Engine.census_batch passes the caps
    ss = [CensusShape(1, 3, 0)] * 600
    assert E.split_census_jobs(ss) == [(0, 256), (256, 512), (512, 600)]
    big = [CensusShape(200, 3, 0)] * 300
    parts = E.split_census_jobs(big)
    per = MAX_PROBE_BYTES // (200 * 32 * 256)
    assert parts[0] == (0, per) and parts[-1][1] == 300 and per < 256
    assert all(hi - lo <= per for lo, hi in parts)


def test_blocks_rule():
    blocks = E.census_batch_blocks_host
    # one job: the single kernel's grid
    assert blocks(1, 1) == 1 and blocks(1, 256) == 1 and blocks(1, 257) == 2
    assert blocks(1, 1 << 16) == 256 and blocks(1, 1 << 20) == 2048
    # 16 jobs: 128 blocks each
    assert blocks(16, 4096) == 16 and blocks(16, 1 << 16) == 128 and blocks(16, 1 << 15) == 128
    # 256 jobs: 8 each, so 4096 candidates (16 tiles) are strided
    assert blocks(256, 4096) == 8 and blocks(256, 2048) == 8 and blocks(256, 1000) == 4
    assert blocks(255, 1 << 16) == 8 and blocks(3, 1 << 20) == 682
    assert blocks(0, 100) == 0 and blocks(4, 0) == 0

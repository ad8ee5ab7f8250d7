"""The host side of mg_walk_batch (csrc/mg_walk_batch.h): the
library exports the new entries, the plan of the batch's device buffer
(mg_walk_batch_plan_host) tiles it with aligned, disjoint regions at the
batch's strides, refuses what it must, and the Python splitting of a job list
under a byte cap covers every job once, in order.  CPU only."""

import ctypes as C

import numpy as np
import pytest

from mythril_amd import engine as E
from mythril_amd.engine import WalkShape

SHARED, REGIONS = E.WALK_BATCH_SHARED, E.WALK_BATCH_JOB_REGIONS
LEAVES, PROBES = REGIONS - 2, REGIONS - 1          # the last two regions of a job


def shape(n_leaves, n_probes, **kw):
    d = dict(n_leaves=n_leaves, n_probes=n_probes, n_roots=3, mask_probe0=0, n_atoms=2, n_code=7,
             n_resid=2, n_entries=0, n_pieces=0, n_srows=0, n_slots=0, n_funcs=0, n_cands=0,
             n_ukeys=0, n_urows=0)
    d.update(kw)
    return WalkShape(**d)


# different leaf and probe counts, one job with every table, one with none
THREE = (shape(5, 9, n_entries=4, n_pieces=6, n_srows=1, n_slots=2, n_funcs=1, n_cands=3,
               n_ukeys=2, n_urows=2, n_resid=3),
         shape(2, 30, n_roots=300, n_atoms=0, n_code=0, n_resid=0),
         shape(11, 4))


def test_library_exports_the_batch_entries():
    lib = E.load_library(check_digest=False)
    for name in ("mg_walk_batch", "mg_walk_batch_plan_host", "mg_walk_batch_shape_ok_host"):
        assert name in E.EXPORTS and getattr(lib, name)


@pytest.mark.parametrize("walkers,lanes,rounds", ((1, 16, 8), (3, 257, 5), (64, 256, 8), (1, 1, 1)))
def test_plan_tiles_the_buffer(walkers, lanes, rounds):
    offs, total = E.walk_batch_plan_host(THREE, walkers, lanes, rounds)
    assert len(offs) == SHARED + 3 * REGIONS
    assert all(int(o) % 256 == 0 for o in offs) and total % 256 == 0
    tot = walkers * lanes
    al = lambda x: (x + 255) & ~255
    # what each region must hold at least (bytes), keyed by its offset
    need = {}
    job = lambda g, k: int(offs[SHARED + g * REGIONS + k])
    for g, s in enumerate(THREE):
        need[job(g, 0)] = walkers * s.n_leaves * 32                      # bases
        need[job(g, 2)] = s.n_roots * 4
        need[job(g, 5)] = s.n_entries * 20
        need[job(g, 13)] = walkers * rounds * 8                          # trace
        need[job(g, LEAVES)] = s.n_leaves * 8 * tot * 4
        need[job(g, PROBES)] = s.n_probes * 8 * tot * 4
    # regions in address order: each ends where the next begins (an empty one
    # shares its offset with its successor), the last at the total
    order = sorted(set(int(o) for o in offs)) + [total]
    assert order[0] == 0
    size = {a: b - a for a, b in zip(order, order[1:])}
    assert sum(size.values()) == total
    for o, n in need.items():
        assert size.get(o, 0) >= n, (o, n)
    # the strides are the maxima over the batch, rounded up to 256 bytes
    leaf_stride = al(max(s.n_leaves for s in THREE) * 8 * tot * 4)
    probe_stride = al(max(s.n_probes for s in THREE) * 8 * tot * 4)
    for g in range(2):
        assert job(g + 1, LEAVES) - job(g, LEAVES) == leaf_stride
        assert job(g + 1, PROBES) - job(g, PROBES) == probe_stride
    assert job(0, PROBES) - job(2, LEAVES) == leaf_stride
    assert total - job(2, PROBES) == probe_stride
    # a job alone needs less: its own counts are the maxima
    _, alone = E.walk_batch_plan_host(THREE[:1], walkers, lanes, rounds)
    assert alone < total


def test_plan_refusals():
    ok = dict(walkers=2, lanes=64, max_rounds=8)
    assert E.walk_batch_plan_host(THREE, **ok) is not None
    assert E.walk_batch_plan_host([], **ok) is None                               # 0 jobs
    cap = E.WALK_BATCH_MAX_JOBS
    assert E.walk_batch_plan_host([THREE[2]] * cap, **ok) is not None
    assert E.walk_batch_plan_host([THREE[2]] * (cap + 1), **ok) is None
    assert E.walk_batch_plan_host(THREE, walkers=65, lanes=64, max_rounds=8) is None
    assert E.walk_batch_plan_host(THREE, walkers=0, lanes=64, max_rounds=8) is None
    assert E.walk_batch_plan_host(THREE, walkers=2, lanes=0, max_rounds=8) is None
    assert E.walk_batch_plan_host(THREE, walkers=2, lanes=(1 << 20) + 1, max_rounds=8) is None
    assert E.walk_batch_plan_host(THREE, walkers=2, lanes=64, max_rounds=0) is None
    assert E.walk_batch_plan_host(THREE, walkers=2, lanes=64, max_rounds=(1 << 16) + 1) is None
    # a total beyond 64 bits: 2^32 - 1 leaves x 32 B x 2^26 lanes x 256 jobs
    huge = shape(0xFFFFFFFF, 0xFFFFFFFF)
    assert E.walk_batch_plan_host([huge] * cap, walkers=64, lanes=1 << 20, max_rounds=8) is None
    # the largest counts one job may have still plan (no overflow on the way)
    big = shape(0xFFFFFFFF, 0xFFFFFFFF, n_ukeys=0xFFFFFFFF, n_pieces=0xFFFFFFFF)
    offs, total = E.walk_batch_plan_host([big], walkers=64, lanes=1 << 19, max_rounds=1 << 16)
    assert 2 * 0xFFFFFFFF * 32 * 64 * (1 << 19) < total < 1 << 64
    # null pointers
    lib = E.load_library(check_digest=False)
    arr = (WalkShape * 1)(THREE[0])
    out = np.zeros(SHARED + REGIONS, dtype=np.uint64)
    n = C.c_uint64()
    assert lib.mg_walk_batch_plan_host(None, 1, 1, 16, 8, out.ctypes.data, C.byref(n)) == -1
    assert lib.mg_walk_batch_plan_host(arr, 1, 1, 16, 8, None, C.byref(n)) == -1
    assert lib.mg_walk_batch_plan_host(arr, 1, 1, 16, 8, out.ctypes.data, None) == -1
    assert lib.mg_walk_batch_plan_host(arr, 1, 1, 16, 8, out.ctypes.data, C.byref(n)) == 0


def test_shape_check():
    lib = E.load_library(check_digest=False)
    ok = lambda s: lib.mg_walk_batch_shape_ok_host(C.byref(s))
    assert all(ok(s) for s in THREE) and not lib.mg_walk_batch_shape_ok_host(None)
    for bad in (shape(0, 4), shape(5, 0), shape(5, 9, n_roots=0), shape(5, 9, n_roots=1025),
                shape(5, 9, n_atoms=1025), shape(5, 9, n_entries=257), shape(5, 9, n_srows=65),
                shape(5, 9, n_slots=65), shape(5, 9, n_funcs=65), shape(5, 9, n_cands=257),
                shape(5, 9, n_urows=129), shape(5, 4, n_resid=3), shape(5, 9, mask_probe0=6),
                shape(5, 9, mask_probe0=0xFFFFFFFF), shape(5, 9, n_resid=0xFFFFFFFF)):
        assert not ok(bad)
    assert ok(shape(5, 9, mask_probe0=5)) and ok(shape(5, 4, n_resid=2))


def test_split_covers_every_job_once_in_order():
    rng = np.random.default_rng(7)
    shapes = [shape(int(rng.integers(1, 12)), int(rng.integers(4, 40))) for _ in range(23)]
    kw = dict(walkers=2, lanes=100, max_rounds=8)
    whole = E.walk_batch_plan_host(shapes, **kw)[1]
    single = [E.walk_batch_plan_host([s], **kw)[1] for s in shapes]
    seen = set()
    for cap in (whole, whole - 1, whole // 2, whole // 5, max(single), 3 * max(single)):
        parts = E.split_walk_jobs(shapes, max_bytes=cap, **kw)
        seen.add(len(parts))
        assert parts[0][0] == 0 and parts[-1][1] == len(shapes)
        assert all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        assert all(lo < hi for lo, hi in parts)
        for lo, hi in parts:
            assert E.walk_batch_plan_host(shapes[lo:hi], **kw)[1] <= cap
            if hi < len(shapes):                        # and one more job would not fit
                assert E.walk_batch_plan_host(shapes[lo:hi + 1], **kw)[1] > cap
    assert 1 in seen and len(seen) >= 4
    assert E.split_walk_jobs(shapes, max_bytes=whole, max_jobs=5, **kw) == \
        [(0, 5), (5, 10), (10, 15), (15, 20), (20, 23)]
    with pytest.raises(E.EngineError, match="walk_batch: job %d alone" % int(np.argmax(single))):
        E.split_walk_jobs(shapes, max_bytes=max(single) - 1, **kw)
    assert E.split_walk_jobs([], max_bytes=1, **kw) == []

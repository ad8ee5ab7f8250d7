"""Witness carry on the GPU (mg_carry_batch, csrc/mg_carry.hip; DESIGN.md
§3.18): the fill kernel against its host lane function bit for bit, the
results against the oracle on the specified candidates on both register
layouts, the unpinned carry against the search, order, the job cap and the
refusals of the C ABI, and get_model / batch_is_possible with
MYTHRIL_GPU_CARRY=1 on hand-built paths and on the stand-in streams."""

import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import census_cases as K
import gen_cases as G
import mythril_amd.model as M
from mythril_amd import carry as CY
from mythril_amd import engine as E
from mythril_amd import workloads as W
from mythril_amd.engine import Gen, default_leafgen, get_engine
from mythril_amd.smt import UGT, ULT, symbol_factory
from oracle import evalref
from oracle import smtlib_ref as R

pytestmark = pytest.mark.gpu

SEED = 0x63617279
FIRST = (1 << 32) + 37                    # above 2^32, no multiple of 64
LADDER = ("ladder", 5)
# case -> (prog_seed, thresholds): both threshold sets in use
CASES = {LADDER: (3, "default"), "rules": (0, "search"), "deep": (5, "search"),
         "flats": (9, "default")}


def built(case, nreg=16):
    """(constraints, eval-form program) of a case of the existing generators."""
    if isinstance(case, tuple):
        return K.masked_program(case, nreg)
    return G.case(case), G.program(case, nreg, "mask")


def leafgen(case, prog):
    return M.search_leafgen(prog) if CASES[case][1] == "search" else default_leafgen(prog)


@functools.lru_cache(maxsize=None)
def loaded(case, nreg=16):
    prog = built(case, nreg)[1]
    ref = built(case)[1]                  # the leaf order and the pool are the 16-slot program's
    assert [(l.name, l.width) for l in prog.leaves] == [(l.name, l.width) for l in ref.leaves]
    assert prog.const_values == ref.const_values
    return get_engine(0, nreg=nreg).load(prog, leafgen(case, prog), prog_seed=CASES[case][0])


def random_pins(case, seed, share):
    """(mask, rows): each leaf pinned with probability ``share`` to a random
    value of its width."""
    prog = built(case)[1]
    rng = np.random.default_rng(seed)
    n = len(prog.leaves)
    mask, rows = np.zeros((n + 31) // 32, dtype=np.uint32), np.zeros((n, 8), dtype=np.uint32)
    for l, leaf in enumerate(prog.leaves):
        if rng.random() < share:
            mask[l >> 5] |= np.uint32(1 << (l & 31))
            v = int.from_bytes(rng.bytes(32), "little") & ((1 << leaf.width) - 1)
            rows[l] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    return mask, rows


def host_fill(case, mask, rows, first, lanes):
    """The specified SoA of a job: mg_carry_fill_host, which tests/test_carry.py
    holds to oracle/gen_ref.py."""
    prog = built(case)[1]
    return E.carry_fill_host(leafgen(case, prog), prog.consts, CASES[case][0], rows, mask, SEED,
                             first, lanes)


@functools.lru_cache(maxsize=None)
def serialized(case):
    cs, prog = built(case)
    return evalref.serialize(cs, prog)


def oracle_result(case, mask, rows, first, lanes):
    """(first true lane or -1, that lane's rows or None) from the oracle."""
    soa = host_fill(case, mask, rows, first, lanes)
    ok = evalref.run_leaves_soa(serialized(case), built(case)[1], soa)
    hit = np.flatnonzero(ok)
    if not hit.size:
        return -1, None
    return int(hit[0]), soa[:, :, int(hit[0])].copy()


def same(got, want):
    assert got[0] == want[0]
    if want[0] < 0:
        assert got[1] is None
    else:
        assert np.array_equal(got[1], want[1])


# ---------------------------------------------------------------------------
# 7. fill parity
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", (1, 63, 64, 65, 256))
def test_fill_equals_the_host_lane_function(lanes):
    eng = get_engine(0)
    cases = (LADDER, "flats", "rules")                  # 3, 274 and 15 leaves: padded rows
    assert [len(built(c)[1].leaves) for c in cases] == [3, 274, 15]
    pins = [random_pins(c, 11 + k, (0.0, 0.5, 0.3)[k]) for k, c in enumerate(cases)]
    assert pins[1][0][1:].any()                         # pinned leaves past mask bit 31
    res = eng.carry_batch([(loaded(c), r, m) for c, (m, r) in zip(cases, pins)], SEED, FIRST,
                          lanes, want_fill=True)
    for c, (m, r), got in zip(cases, pins, res):
        want = host_fill(c, m, r, FIRST, lanes)
        assert got[2].shape == want.shape == (len(built(c)[1].leaves), 8, lanes)
        assert np.array_equal(got[2], want), (c, lanes)
        # and the returned rows are a column of the region
        if got[0] >= 0:
            assert np.array_equal(got[1], want[:, :, got[0]])


# ---------------------------------------------------------------------------
# 8. result parity against the oracle, 9. the unpinned carry is the search
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ladder_model():
    """Rows of a model of the ladder, found by the oracle among the generator's
    candidates."""
    n = len(built(LADDER)[1].leaves)
    none = np.zeros((n + 31) // 32, dtype=np.uint32)
    first, rows = oracle_result(LADDER, none, np.zeros((n, 8), dtype=np.uint32), 0, 4096)
    assert first >= 0
    return rows


def four_kinds():
    """(case, mask, rows) of: a known model pinned; the same with one pinned
    leaf changed so that a root fails; a mixed job; a job with nothing pinned;
    then mixed and unpinned jobs of other leaf counts."""
    prog = built(LADDER)[1]
    names = [l.source for l in prog.leaves]
    model = ladder_model()
    every = np.array([(1 << len(names)) - 1], dtype=np.uint32)
    broken = model.copy()
    broken[names.index("y")] = 0
    broken[names.index("y"), 0] = 0xFFFF               # y < 2^15 fails
    only_x = np.array([1 << names.index("x")], dtype=np.uint32)
    none = np.zeros(1, dtype=np.uint32)
    jobs = [(LADDER, every, model), (LADDER, every, broken), (LADDER, only_x, model),
            (LADDER, none, model)]
    for k, c in enumerate(("rules", "deep", "flats")):
        jobs.append((c,) + random_pins(c, 31 + k, 0.5))
        jobs.append((c,) + random_pins(c, 41 + k, 0.0))
    return jobs


@pytest.mark.parametrize("nreg", (16, 11))
def test_results_equal_the_oracle_on_the_specified_candidates(nreg):
    eng = get_engine(0, nreg=nreg)
    jobs = four_kinds()
    for lanes, first in ((256, FIRST), (65, 0)):
        res = eng.carry_batch([(loaded(c, nreg), r, m) for c, m, r in jobs], SEED, first, lanes)
        want = [oracle_result(c, m, r, first, lanes) for c, m, r in jobs]
        for k, (g, w) in enumerate(zip(res, want)):
            same(g, w)
        assert res[0][0] == 0 and np.array_equal(res[0][1], ladder_model())
        assert res[1] == (-1, None)
        assert res[2][0] >= 0 and res[3][0] >= 0
    assert eng.last_kernel_ms() > 0
    # zero rows where there is no lane, through the raw ABI
    arr = (E.CarryJob * 2)()
    keep = []
    for i, (c, m, r) in enumerate(jobs[:2]):
        keep.append((np.ascontiguousarray(r), np.ascontiguousarray(m)))
        arr[i].prog, arr[i].pin_rows, arr[i].pin_mask = (loaded(c, nreg).handle, E._ptr(keep[i][0]),
                                                         E._ptr(keep[i][1]))
    first = np.full(2, 7, dtype=np.int64)
    out = np.full((2, 5, 8), 0xAB, dtype=np.uint32)
    g = Gen(SEED, 0)
    assert eng.lib.mg_carry_batch(eng._ctx, arr, 2, C.byref(g), 1, E._ptr(first), E._ptr(out), 5,
                                  None) == 0
    assert first.tolist() == [0, -1]
    assert np.array_equal(out[0, :3], ladder_model()) and not out[0, 3:].any() and not out[1].any()


@pytest.mark.parametrize("nreg", (16, 11))
def test_with_nothing_pinned_the_carry_is_the_search(nreg):
    eng = get_engine(0, nreg=nreg)
    first = (1 << 33) + 64                              # the search's launches start at a multiple of 64
    found = 0
    for case in (LADDER, "rules", "deep"):
        lp = loaded(case, nreg)
        n = len(lp.program.leaves)
        none, rows = np.zeros((n + 31) // 32, dtype=np.uint32), np.zeros((n, 8), dtype=np.uint32)
        for lanes in (256, 1000):
            (got,) = eng.carry_batch([(lp, rows, none)], SEED, first, lanes)
            idx, wit = eng.search(lp, SEED, lanes, first)
            assert got[0] == (idx - first if idx >= 0 else -1), (case, lanes)
            if idx >= 0:
                assert np.array_equal(got[1], wit)
                found += 1
    assert found >= 2


# ---------------------------------------------------------------------------
# 10. order and refusals
# ---------------------------------------------------------------------------

def test_order_the_job_cap_and_the_refusals():
    eng = get_engine(0)
    jobs = four_kinds()
    args = [(loaded(c), r, m) for c, m, r in jobs]
    res = eng.carry_batch(args, SEED, FIRST, 64)
    back = eng.carry_batch(args[::-1], SEED, FIRST, 64)
    for a, b in zip(res, back[::-1]):
        same(a, b)
    assert eng.carry_batch([], SEED, FIRST, 64) == []
    # 257 jobs: Engine.carry_batch splits, the raw ABI refuses
    many = (args[:4] * 65)[:257]
    got = eng.carry_batch(many, SEED, FIRST, 64)
    assert len(got) == 257
    for k, g in enumerate(got):
        same(g, res[k % 4])
    ms = eng.last_kernel_ms()

    def raw(n_jobs, lanes, max_leaves, handles=None, rows=True, mask=True, first=True, out=True,
            gen=True, jobs_ptr=True, ctx=None):
        arr = (E.CarryJob * max(1, n_jobs))()
        for i in range(n_jobs):
            lp, r, m = many[i]
            arr[i].prog = handles[i] if handles else lp.handle
            arr[i].pin_rows = E._ptr(r) if rows else None
            arr[i].pin_mask = E._ptr(m) if mask else None
        f = np.zeros(max(1, n_jobs), dtype=np.int64)
        o = np.zeros((max(1, n_jobs), max(1, max_leaves), 8), dtype=np.uint32)
        g = Gen(SEED, FIRST)
        rc = eng.lib.mg_carry_batch(eng._ctx, arr if jobs_ptr else None, n_jobs,
                                    C.byref(g) if gen else None, lanes, E._ptr(f) if first else None,
                                    E._ptr(o) if out else None, max_leaves, None)
        return rc, eng.lib.mg_last_error(eng._ctx)

    assert raw(257, 64, 3) == (-1, b"carry_batch: 257 jobs outside 1..256")
    assert raw(0, 64, 3) == (-1, b"carry_batch: 0 jobs outside 1..256")
    assert raw(2, 0, 3) == (-1, b"carry_batch: 0 lanes outside 1..1048576")
    assert raw(2, (1 << 20) + 1, 3) == (-1, b"carry_batch: 1048577 lanes outside 1..1048576")
    for kw in ({"first": False}, {"out": False}, {"gen": False}, {"jobs_ptr": False}):
        assert raw(2, 64, 3, **kw) == (-1, b"carry_batch: null argument")
    assert raw(2, 64, 3, rows=False) == (-1, b"carry_batch: job 0: null pin rows or pin mask")
    assert raw(2, 64, 3, mask=False) == (-1, b"carry_batch: job 0: null pin rows or pin mask")
    assert raw(2, 64, 3, handles=[many[0][0].handle, None]) == \
        (-1, b"carry_batch: job 1: null program")
    other = loaded(LADDER, 11)                          # a program of the 11-slot context
    assert raw(2, 64, 3, handles=[many[0][0].handle, other.handle]) == \
        (-1, b"carry_batch: job 1: a program of another context")
    assert raw(2, 64, 2) == (-1, b"carry_batch: job 0: 3 leaves above max_leaves 2")
    rc, why = raw(2, 64, (1 << 20) + 1)
    assert rc == -1 and why.startswith(b"carry_batch: max_leaves")
    # 256 jobs of 274 leaves at 2^20 lanes: above the buffer the call may take
    flats = loaded("flats")
    m, r = random_pins("flats", 1, 0.5)
    with pytest.raises(E.EngineError, match="bytes needed for 256 jobs"):
        eng.carry_batch([(flats, r, m)] * 256, SEED, 0, 1 << 20)
    assert eng.last_kernel_ms() == ms                   # nothing was launched
    # and the context is still usable
    again = eng.carry_batch(args, SEED, FIRST, 64)
    for a, b in zip(res, again):
        same(a, b)


# ---------------------------------------------------------------------------
# 11. end to end on hand-built paths
# ---------------------------------------------------------------------------

BVV = symbol_factory.BitVecVal
BVS = symbol_factory.BitVecSym


@pytest.fixture
def knob(monkeypatch):
    """MYTHRIL_GPU_CARRY=1 on fresh memos and statistics."""
    def fresh(on=True):
        monkeypatch.setattr(M, "CARRY", on)
        M.clear_search_memos()
        M.get_model.cache_clear()
        M._batch_witness.clear()
        M._gpu_missed.clear()
        M.stats.reset_gpu()
    M.time_handler.start_execution(3600)
    fresh()
    yield fresh
    monkeypatch.setattr(M, "CARRY", False)
    M.clear_search_memos()
    M.get_model.cache_clear()
    M.stats.reset_gpu()


def model_of(constraints):
    """get_model's model, oracle-checked; or the exception type of a miss."""
    try:
        m = M.get_model(tuple(constraints), enforce_execution_time=False)
    except (M.SolverUnavailable, M.UnsatError) as e:
        return type(e)
    a = m.assignment
    assert R.eval_constraints([c.raw for c in constraints], R.Assignment(a.vars, a.arrays,
                                                                         a.funcs)) == 1
    return a


def search_key(constraints):
    (b,) = M.dependence_buckets(M._raw_nodes(constraints))
    return (tuple(n.id for n in b), ())


def test_a_child_the_parent_model_satisfies_is_a_one_candidate_carry_hit(knob):
    x = BVS("carry_x", 256)
    parent = [x == BVV(7, 256)]
    child = parent + [ULT(x, BVV(100, 256))]
    assert model_of(parent).vars["carry_x"] == 7
    assert search_key(parent) in M._SEARCH_CACHE and M._group_key(M._raw_nodes(parent)) in M._group_hit
    s = M.stats
    assert (s.carry_exact, s.carry_attempts, s.carry_hits) == (0, 0, 0)
    a = model_of(child)
    assert a.vars["carry_x"] == 7
    assert (s.carry_exact, s.carry_attempts, s.carry_hits, s.carry_candidates) == (0, 1, 1, 1)
    assert search_key(child) not in M._SEARCH_CACHE        # no solve-mode compile of the child
    assert s.gpu_hits == 2
    # the child is remembered too: its own extension carries from it
    grand = child + [UGT(x, BVV(3, 256))]
    assert model_of(grand).vars["carry_x"] == 7
    assert (s.carry_attempts, s.carry_hits, s.carry_candidates) == (2, 2, 2)
    assert "GPU carry: exact: 0 attempts: 2 hits: 2 candidates: 2" in repr(s)


def test_a_child_with_a_fresh_symbol_keeps_the_parent_value(knob):
    x, y = BVS("carry_x", 256), BVS("carry_y", 256)
    parent = [x == BVV(7, 256)]
    assert model_of(parent).vars["carry_x"] == 7
    s = M.stats
    # y > 3 shares no symbol with the parent: the query splits into the parent's
    # group, answered from the memo without a launch, and a group of its own,
    # which extends nothing and is searched
    a = model_of(parent + [UGT(y, BVV(3, 256))])
    assert a.vars["carry_x"] == 7 and a.vars["carry_y"] > 3
    assert (s.carry_exact, s.carry_attempts, s.carry_hits) == (1, 0, 0)
    # a fresh symbol inside the parent's group: x pinned, y from the generator
    child = parent + [UGT(y, x)]
    a = model_of(child)
    assert a.vars["carry_x"] == 7 and a.vars["carry_y"] > 7
    assert (s.carry_exact, s.carry_attempts, s.carry_hits) == (1, 1, 1)
    assert s.carry_candidates == CY.CARRY_LANES
    assert search_key(child) not in M._SEARCH_CACHE


@pytest.mark.parametrize("refute", (True, False))
def test_a_child_the_parent_model_fails_takes_the_route_of_the_knob_off(knob, monkeypatch, refute):
    # with the host refutation on, x == 7 and x > 100 never reach the carry (it
    # comes after the refutation); with it off the carry is tried and misses
    monkeypatch.setattr(M, "REFUTE", refute)
    x = BVS("carry_x", 256)
    parent = [x == BVV(7, 256)]
    child = parent + [UGT(x, BVV(100, 256))]
    outcome = {}
    for on in (False, True):
        knob(on)
        assert model_of(parent).vars["carry_x"] == 7
        outcome[on] = model_of(child)
        s = M.stats
        want = (0, 0) if refute or not on else (1, 0)
        assert (s.carry_attempts, s.carry_hits) == want
        assert s.refuted == (1 if refute else 0)
        if not refute:
            assert search_key(child) in M._SEARCH_CACHE    # the miss went on to the search
    assert outcome[True] is outcome[False] is M.SolverUnavailable
    # a satisfiable child the parent's model fails: the same model either way
    p2 = [ULT(x, BVV(50, 256))]
    c2 = p2 + [UGT(x, BVV(20, 256))]
    models = {}
    for on in (False, True):
        knob(on)
        first = model_of(p2)
        got = model_of(c2)
        models[on] = (first.vars["carry_x"], got if isinstance(got, type) else got.vars["carry_x"])
    assert models[True][0] == models[False][0]
    if models[True][0] > 20:                                # the parent's model carries
        assert M.stats.carry_hits == 1 and models[True][1] == models[True][0]
    else:
        assert (M.stats.carry_attempts, M.stats.carry_hits) == (1, 0)
        assert models[True] == models[False]


def test_posing_the_parent_twice_is_an_exact_hit_without_a_launch(knob):
    x = BVS("carry_x", 256)
    parent = [x == BVV(7, 256)]
    assert model_of(parent).vars["carry_x"] == 7
    s = M.stats
    kernel, cands, load = s.kernel_time, s.gpu_candidates, s.phase["load"]
    M.get_model.cache_clear()                               # (the whole-query cache would answer)
    assert model_of(parent).vars["carry_x"] == 7
    assert (s.carry_exact, s.carry_attempts) == (1, 0)
    assert (s.kernel_time, s.gpu_candidates, s.phase["load"]) == (kernel, cands, load)
    # batch_is_possible: the exact repeat and two extensions in one carry call
    M.get_model.cache_clear()
    sets = [tuple(parent), tuple(parent + [ULT(x, BVV(100, 256))]),
            tuple(parent + [ULT(x, BVV(9, 256))])]
    assert M.batch_is_possible(sets, enforce_execution_time=False) == [True, True, True]
    assert (s.carry_exact, s.carry_attempts, s.carry_hits) == (2, 2, 2)
    assert s.gpu_candidates == cands                        # nothing was searched


# ---------------------------------------------------------------------------
# 12. streams, knob on against knob off
# ---------------------------------------------------------------------------

HERE = os.path.dirname(os.path.abspath(__file__))
LABELS = json.load(open(os.path.join(HERE, "golden", "recall_labels.json")))


def run_stream(qs):
    out = []
    for q in qs:
        try:
            m = M.get_model(tuple(q), enforce_execution_time=False)
            out.append(m.assignment)
        except (M.SolverUnavailable, M.UnsatError):
            out.append(None)
    return out


@pytest.mark.parametrize("stream", ("c4", "c5"))
def test_streams_lose_no_model_and_gain_no_wrong_one(knob, stream):
    qs = W.queries(stream, LABELS["n"])[:64]
    unsat = {r["i"] for r in LABELS["streams"].get(stream, ()) if r["label"] == "unsat"}
    knob(False)
    off = run_stream(qs)
    knob(True)
    on = run_stream(qs)
    s = M.stats
    print("carry %s: models off %d on %d; exact %d attempts %d hits %d" % (
        stream, sum(a is not None for a in off), sum(a is not None for a in on), s.carry_exact,
        s.carry_attempts, s.carry_hits))
    for i, (q, a, b) in enumerate(zip(qs, off, on)):
        if a is not None:
            assert b is not None, (stream, i)
        if b is not None:
            assert R.eval_constraints(list(q), R.Assignment(b.vars, b.arrays, b.funcs)) == 1, \
                (stream, i)
            assert i not in unsat, (stream, i)
    assert s.carry_exact > 0

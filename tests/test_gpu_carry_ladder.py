"""The pin ladder of the witness carry on the GPU (mg_carry_ladder,
csrc/mg_carry_ladder.hip): the rung fill kernel against its
host lane function bit for bit, first / rung / leaves against the oracle on the
specified columns on both register layouts, one rung against mg_carry_batch,
the refusals of the C ABI, and get_model with MYTHRIL_GPU_CARRY=2 on a
hand-built calldata path and on the stand-in streams."""

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
from mythril_amd.assign import lookup, unpack
from mythril_amd.engine import Gen, default_leafgen, get_engine
from mythril_amd.smt import Array, symbol_factory
from oracle import evalref
from oracle import smtlib_ref as R

pytestmark = pytest.mark.gpu

SEED = 0x6C616464
FIRST = (1 << 32) + 37                    # above 2^32, no multiple of 64
LADDER = ("ladder", 5)
# case -> (prog_seed, thresholds): both threshold sets in use
CASES = {LADDER: (3, "default"), "rules": (0, "search"), "flats": (9, "default")}


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


def random_rungs(case, seed, n_rungs, share):
    """(masks, rows): ``n_rungs`` masks, each leaf pinned on a rung with
    probability ``share``, and a random row of its width per leaf."""
    prog = built(case)[1]
    rng = np.random.default_rng(seed)
    n = len(prog.leaves)
    masks = np.zeros((n_rungs, (n + 31) // 32), dtype=np.uint32)
    rows = np.zeros((n, 8), dtype=np.uint32)
    for l, leaf in enumerate(prog.leaves):
        v = int.from_bytes(rng.bytes(32), "little") & ((1 << leaf.width) - 1)
        rows[l] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
        for r in range(n_rungs):
            if rng.random() < share:
                masks[r, l >> 5] |= np.uint32(1 << (l & 31))
    return masks, rows


def host_fill(case, masks, rows, first, lanes, cols=None):
    """The specified SoA of a job: mg_carry_fill_rungs_host, which
    tests/test_carry_ladder.py holds to mg_carry_fill_host rung by rung."""
    prog = built(case)[1]
    return E.carry_fill_rungs_host(leafgen(case, prog), prog.consts, CASES[case][0], rows, masks,
                                   SEED, first, lanes, cols=cols)


@functools.lru_cache(maxsize=None)
def serialized(case):
    cs, prog = built(case)
    return evalref.serialize(cs, prog)


def oracle_result(case, masks, rows, first, lanes, cols=None):
    """(first true column or -1, its rung or -1, its rows or None) from the
    oracle on the specified columns."""
    soa = host_fill(case, masks, rows, first, lanes, cols)
    ok = evalref.run_leaves_soa(serialized(case), built(case)[1], soa)
    hit = np.flatnonzero(ok)
    if not hit.size:
        return -1, -1, None
    c = int(hit[0])
    return c, min(c // lanes, masks.shape[0] - 1), soa[:, :, c].copy()


def same(got, want):
    assert got[:2] == want[:2]
    if want[0] < 0:
        assert got[2] is None
    else:
        assert np.array_equal(got[2], want[2])


# ---------------------------------------------------------------------------
# fill parity
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", (1, 63, 65, 256))
def test_fill_equals_the_host_lane_function(lanes):
    eng = get_engine(0)
    cases, n_rungs = (LADDER, "flats", "rules"), (3, 1, 2)   # 3, 274 and 15 leaves: padded rows
    assert [len(built(c)[1].leaves) for c in cases] == [3, 274, 15]
    pins = [random_rungs(c, 11 + k, n_rungs[k], (0.4, 0.5, 0.3)[k]) for k, c in enumerate(cases)]
    assert pins[1][0][0, 1:].any()                        # pinned leaves past mask bit 31
    assert len({m.tobytes() for m in pins[0][0]}) == 3    # the rungs differ
    res = eng.carry_ladder([(loaded(c), r, m) for c, (m, r) in zip(cases, pins)], SEED, FIRST,
                           lanes, want_fill=True)
    cols = 3 * lanes
    for c, (m, r), got in zip(cases, pins, res):
        want = host_fill(c, m, r, FIRST, lanes, cols)     # the surplus repeats the last rung
        assert got[3].shape == want.shape == (len(built(c)[1].leaves), 8, cols)
        assert np.array_equal(got[3], want), (c, lanes)
        # and the returned rows are a column of the region, on the rung reported
        if got[0] >= 0:
            assert np.array_equal(got[2], want[:, :, got[0]])
            assert got[1] == min(got[0] // lanes, m.shape[0] - 1)
        else:
            assert got[1] == -1 and got[2] is None


# ---------------------------------------------------------------------------
# result parity against the oracle
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ladder_model():
    """Rows of a model of the ladder, found by the oracle among the generator's
    candidates."""
    n = len(built(LADDER)[1].leaves)
    first, _, rows = oracle_result(LADDER, np.zeros((1, 1), dtype=np.uint32),
                                   np.zeros((n, 8), dtype=np.uint32), 0, 4096)
    assert first >= 0
    return rows


def three_outcomes():
    """(case, masks, rows) of: a known model with everything pinned on rung 0;
    the model with y broken, everything pinned on rung 0 and only x on rung 1;
    the same with y pinned on every rung (y < 2^15 fails whatever x is)."""
    prog = built(LADDER)[1]
    names = [l.source for l in prog.leaves]
    model = ladder_model()
    bits = lambda *ns: [sum(1 << names.index(n) for n in ns)]       # noqa: E731
    every = bits(*set(names))
    broken = model.copy()
    broken[names.index("y")] = 0
    broken[names.index("y"), 0] = 0xFFFF
    u32 = lambda rows: np.array(rows, dtype=np.uint32)              # noqa: E731
    return [(LADDER, u32([every, bits("x"), [0]]), model),
            (LADDER, u32([every, bits("x")]), broken),
            (LADDER, u32([every, bits("y")]), broken)]


@pytest.mark.parametrize("nreg", (16, 11))
def test_first_rung_and_leaves_equal_the_oracle_on_the_specified_columns(nreg):
    eng = get_engine(0, nreg=nreg)
    jobs = three_outcomes()
    for lanes, first in ((65, 0), (256, FIRST)):
        # the oracle alone: rung 0 hits, rung 0 misses and rung 1 hits, no rung hits
        want = [oracle_result(c, m, r, first, lanes, 3 * lanes) for c, m, r in jobs]
        assert want[0][:2] == (0, 0) and np.array_equal(want[0][2], ladder_model())
        assert want[1][1] == 1 and lanes <= want[1][0] < lanes + 65
        assert want[2] == (-1, -1, None)
        res = eng.carry_ladder([(loaded(c, nreg), r, m) for c, m, r in jobs], SEED, first, lanes)
        for g, w in zip(res, want):
            same(g, w)
        # a batch of its own has its own R: the same rung, candidate and rows
        (alone,) = eng.carry_ladder([(loaded(LADDER, nreg), jobs[1][2], jobs[1][1])], SEED, first,
                                    lanes)
        same(alone, want[1])
    assert eng.last_kernel_ms() > 0
    # zero rows and -1 where there is no column, through the raw ABI
    arr = (E.CarryLadderJob * 2)()
    keep = [(np.ascontiguousarray(r), np.ascontiguousarray(m)) for _, m, r in (jobs[0], jobs[2])]
    for i, (r, m) in enumerate(keep):
        arr[i].prog, arr[i].pin_rows, arr[i].pin_masks = (loaded(LADDER, nreg).handle, E._ptr(r),
                                                          E._ptr(m))
        arr[i].n_rungs = m.shape[0]
    first, rung = np.full(2, 7, dtype=np.int64), np.full(2, 7, dtype=np.int64)
    out = np.full((2, 5, 8), 0xAB, dtype=np.uint32)
    g = Gen(SEED, 0)
    assert eng.lib.mg_carry_ladder(eng._ctx, arr, 2, C.byref(g), 1, E._ptr(first), E._ptr(rung),
                                   E._ptr(out), 5, None) == 0
    assert first.tolist() == [0, -1] and rung.tolist() == [0, -1]
    assert np.array_equal(out[0, :3], ladder_model()) and not out[0, 3:].any() and not out[1].any()


# ---------------------------------------------------------------------------
# one rung is mg_carry_batch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", (65, 256))
def test_one_rung_is_carry_batch(lanes):
    eng = get_engine(0)
    jobs = [(c,) + random_rungs(c, 31 + k, 1, share)
            for k, (c, share) in enumerate(((LADDER, 0.3), ("rules", 0.5), ("rules", 0.0),
                                            ("flats", 0.5), (LADDER, 0.0)))]
    # and the mask of carry.pins on a carried assignment
    prog = built(LADDER)[1]
    asg = unpack(prog, ladder_model())
    del asg.vars["y"]
    mask, rows = CY.pins(prog, asg)
    assert CY.n_free(prog, mask) == 1
    jobs.append((LADDER, mask[None, :], rows))
    res = eng.carry_ladder([(loaded(c), r, m) for c, m, r in jobs], SEED, FIRST, lanes)
    old = eng.carry_batch([(loaded(c), r, m[0]) for c, m, r in jobs], SEED, FIRST, lanes)
    hits = 0
    for (first, rung, leaves), (f0, l0) in zip(res, old):
        assert first == f0 and rung == (0 if f0 >= 0 else -1)
        if f0 >= 0:
            assert np.array_equal(leaves, l0)
            hits += 1
        else:
            assert leaves is None
    assert hits >= 2 and res[-1][0] >= 0


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def test_the_job_cap_and_the_refusals():
    eng = get_engine(0)
    jobs = three_outcomes()
    args = [(loaded(c), r, m) for c, m, r in jobs]
    res = eng.carry_ladder(args, SEED, FIRST, 64)
    assert eng.carry_ladder([], SEED, FIRST, 64) == []
    # 257 jobs: Engine.carry_ladder splits, the raw ABI refuses
    many = (args * 86)[:257]
    got = eng.carry_ladder(many, SEED, FIRST, 64)
    assert len(got) == 257
    for k, g in enumerate(got):
        same(g, res[k % 3])
    ms = eng.last_kernel_ms()
    # wrong shapes never reach the library
    for bad in ((args[0][0], args[0][1][:2], args[0][2]), (args[0][0], args[0][1], args[0][2][0]),
                (args[0][0], args[0][1], np.zeros((9, 1), dtype=np.uint32)),
                (args[0][0], args[0][1], np.zeros((0, 1), dtype=np.uint32)),
                (args[0][0], args[0][1], np.zeros((2, 2), dtype=np.uint32))):
        with pytest.raises(ValueError):
            eng.carry_ladder([bad], SEED, FIRST, 64)

    def raw(n_jobs, lanes, max_leaves, handles=None, rows=True, masks=True, first=True, rung=True,
            out=True, gen=True, jobs_ptr=True, n_rungs=None):
        arr = (E.CarryLadderJob * max(1, n_jobs))()
        for i in range(n_jobs):
            lp, r, m = many[i]
            arr[i].prog = handles[i] if handles else lp.handle
            arr[i].pin_rows = E._ptr(r) if rows else None
            arr[i].pin_masks = E._ptr(m) if masks else None
            arr[i].n_rungs = m.shape[0] if n_rungs is None else n_rungs[i]
        f = np.zeros(max(1, n_jobs), dtype=np.int64)
        q = np.zeros(max(1, n_jobs), dtype=np.int64)
        o = np.zeros((max(1, n_jobs), max(1, min(max_leaves, 8)), 8), dtype=np.uint32)
        g = Gen(SEED, FIRST)
        rc = eng.lib.mg_carry_ladder(eng._ctx, arr if jobs_ptr else None, n_jobs,
                                     C.byref(g) if gen else None, lanes,
                                     E._ptr(f) if first else None, E._ptr(q) if rung else None,
                                     E._ptr(o) if out else None, max_leaves, None)
        return rc, eng.lib.mg_last_error(eng._ctx)

    # what mg_carry_batch refuses
    assert raw(257, 64, 3) == (-1, b"carry_ladder: 257 jobs outside 1..256")
    assert raw(0, 64, 3) == (-1, b"carry_ladder: 0 jobs outside 1..256")
    assert raw(2, 0, 3) == (-1, b"carry_ladder: 0 lanes outside 1..1048576")
    assert raw(2, (1 << 20) + 1, 3) == (-1, b"carry_ladder: 1048577 lanes outside 1..1048576")
    for kw in ({"first": False}, {"rung": False}, {"out": False}, {"gen": False},
               {"jobs_ptr": False}):
        assert raw(2, 64, 3, **kw) == (-1, b"carry_ladder: null argument")
    assert raw(2, 64, 3, rows=False) == (-1, b"carry_ladder: job 0: null pin rows or pin masks")
    assert raw(2, 64, 3, masks=False) == (-1, b"carry_ladder: job 0: null pin rows or pin masks")
    assert raw(2, 64, 3, handles=[many[0][0].handle, None]) == \
        (-1, b"carry_ladder: job 1: null program")
    other = loaded(LADDER, 11)                          # a program of the 11-slot context
    assert raw(2, 64, 3, handles=[many[0][0].handle, other.handle]) == \
        (-1, b"carry_ladder: job 1: a program of another context")
    assert raw(2, 64, 2) == (-1, b"carry_ladder: job 0: 3 leaves above max_leaves 2")
    rc, why = raw(2, 64, (1 << 20) + 1)
    assert rc == -1 and why.startswith(b"carry_ladder: max_leaves")
    # the ladder's own: n_rungs outside 1..8, R x lanes above 2^20
    assert raw(2, 64, 3, n_rungs=[3, 0]) == (-1, b"carry_ladder: job 1: 0 rungs outside 1..8")
    assert raw(2, 64, 3, n_rungs=[9, 2]) == (-1, b"carry_ladder: job 0: 9 rungs outside 1..8")
    assert raw(3, (1 << 20) // 3 + 1, 3) == \
        (-1, b"carry_ladder: 3 rungs of 349526 lanes above 1048576 columns")
    assert raw(1, 1 << 20, 3, n_rungs=[2]) == \
        (-1, b"carry_ladder: 2 rungs of 1048576 lanes above 1048576 columns")
    # 256 jobs of 274 leaves at 2^17 lanes x 8 rungs: above the buffer the call may take
    flats = loaded("flats")
    m, r = random_rungs("flats", 1, 8, 0.5)
    with pytest.raises(E.EngineError, match="bytes needed for 256 jobs"):
        eng.carry_ladder([(flats, r, m)] * 256, SEED, 0, 1 << 17)
    assert eng.last_kernel_ms() == ms                   # nothing was launched
    # and the context is still usable
    again = eng.carry_ladder(args, SEED, FIRST, 64)
    for a, b in zip(res, again):
        same(a, b)


# ---------------------------------------------------------------------------
# end to end: a child that reads a calldata byte the parent never read
# ---------------------------------------------------------------------------

BVV = symbol_factory.BitVecVal


@pytest.fixture
def knob(monkeypatch):
    """MYTHRIL_GPU_CARRY at a value of choice on fresh memos and statistics."""
    def fresh(value):
        monkeypatch.setattr(M, "CARRY", value)
        M.clear_search_memos()
        M.get_model.cache_clear()
        M._batch_witness.clear()
        M._gpu_missed.clear()
        M.stats.reset_gpu()
    M.time_handler.start_execution(3600)
    yield fresh
    monkeypatch.setattr(M, "CARRY", False)
    M.clear_search_memos()
    M.get_model.cache_clear()
    M.stats.reset_gpu()


def model_of(constraints):
    """get_model's model, oracle-checked."""
    m = M.get_model(tuple(constraints), enforce_execution_time=False)
    a = m.assignment
    assert R.eval_constraints([c.raw for c in constraints], R.Assignment(a.vars, a.arrays,
                                                                         a.funcs)) == 1
    return a


def search_key(constraints):
    (b,) = M.dependence_buckets(M._raw_nodes(constraints))
    return (tuple(n.id for n in b), ())


BYTE4 = 0x77


def test_the_read_rung_carries_a_child_that_reads_a_byte_the_parent_never_read(knob):
    cd = Array("ladder_calldata", 256, 8)
    parent = [cd[BVV(k, 256)] == BVV(0xA0 + k, 8) for k in range(4)]
    child = parent + [cd[BVV(4, 256)] == BVV(BYTE4, 8)]
    (nodes,) = M.dependence_buckets(M._raw_nodes(child))       # one group: nothing splits off
    old, new = CY.split_nodes(nodes, [M._group_key(M._raw_nodes(parent))])
    assert len(old) == 4 and len(new) == 1
    s = M.stats
    witnesses = {}
    for value in (True, "ladder"):
        knob(value)
        w = model_of(parent)
        witnesses[value] = w
        tab = w.arrays["ladder_calldata"]
        assert [lookup(tab, k) for k in range(4)] == [0xA0, 0xA1, 0xA2, 0xA3]
        # the parent's witness does not meet the child: its byte 4 was a don't-care
        assert lookup(tab, 4) != BYTE4
        assert (s.carry_attempts, s.carry_hits, s.carry_gated, s.refuted) == (0, 0, 0, 0)
        if value == "ladder":
            # on the CPU: under this witness rung "all" has no satisfying column and rung
            # "read" has one within CARRY_LANES
            prog = CY.compile_eval_ck(nodes, w)
            rows, masks = CY.rungs(prog, w, old, new)
            assert masks.shape[0] == 3
            soa = E.carry_fill_rungs_host(M.search_leafgen(prog), prog.consts, 0, rows, masks,
                                          M.SEARCH_SEED, 0, CY.CARRY_LANES)
            ok = evalref.run_leaves_soa(evalref.serialize(nodes, prog), prog, soa)
            hit = np.flatnonzero(ok)
            assert hit.size and CY.CARRY_LANES <= hit[0] < 2 * CY.CARRY_LANES
        a = model_of(child)
        assert lookup(a.arrays["ladder_calldata"], 4) == BYTE4
        if value is True:
            # knob 1: every leaf of the table is pinned; tried, missed, searched
            assert (s.carry_attempts, s.carry_hits, s.carry_candidates) == (1, 0, 1)
            assert search_key(child) in M._SEARCH_CACHE
            assert s.carry_rung_hits == [0, 0, 0]
        else:
            # knob 2: a hit on rung "read", and no solve-mode compile of the child
            assert (s.carry_attempts, s.carry_hits) == (1, 1)
            assert s.carry_rung_hits == [0, 1, 0]
            assert s.carry_candidates == 1 + 2 * CY.CARRY_LANES
            assert search_key(child) not in M._SEARCH_CACHE
            assert [lookup(a.arrays["ladder_calldata"], k) for k in range(4)] == \
                [0xA0, 0xA1, 0xA2, 0xA3]
            assert "rung hits: 0/1/0" in repr(s)
    assert repr(witnesses[True]) == repr(witnesses["ladder"])  # the same parent witness


# ---------------------------------------------------------------------------
# streams, knob 2 against knob off
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
def test_streams_lose_no_model_and_gain_no_wrong_one_under_the_ladder(knob, stream):
    qs = W.queries(stream, LABELS["n"])[:64]
    unsat = {r["i"] for r in LABELS["streams"].get(stream, ()) if r["label"] == "unsat"}
    knob(False)
    off = run_stream(qs)
    knob("ladder")
    on = run_stream(qs)
    s = M.stats
    print("ladder %s: models off %d on %d; exact %d attempts %d hits %d rungs %s gated %d" % (
        stream, sum(a is not None for a in off), sum(a is not None for a in on), s.carry_exact,
        s.carry_attempts, s.carry_hits, s.carry_rung_hits, s.carry_gated))
    for i, (q, a, b) in enumerate(zip(qs, off, on)):
        if a is not None:
            assert b is not None, (stream, i)
        if b is not None:
            assert R.eval_constraints(list(q), R.Assignment(b.vars, b.arrays, b.funcs)) == 1, \
                (stream, i)
            assert i not in unsat, (stream, i)
    assert s.carry_exact > 0

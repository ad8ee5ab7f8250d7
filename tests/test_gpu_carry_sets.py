"""Witness sets on the pin ladder on the GPU (mg_carry_ladder_sets,
csrc/mg_carry_sets.hip): the set fill kernel against its host
lane function bit for bit, first / rung / leaves against the oracle on the
specified columns on both register layouts, one set against mg_carry_ladder, the
refusals of the C ABI, and get_model with MYTHRIL_GPU_CARRY=4 on a hand-built
path whose second remembered witness is the one that carries, and on the
stand-in streams."""

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
from mythril_amd.assign import Assignment
from mythril_amd.engine import Gen, default_leafgen, get_engine
from mythril_amd.smt import UGT, ULT, symbol_factory
from oracle import evalref
from oracle import smtlib_ref as R

pytestmark = pytest.mark.gpu

SEED = 0x73657473
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


def random_sets(case, seed, n_rungs, n_sets, share):
    """(rows, masks, rung_set): ``n_sets`` random row sets, ``n_rungs`` masks
    that pin a leaf with probability ``share`` and a random set per rung, the
    last set in use."""
    prog = built(case)[1]
    rng = np.random.default_rng(seed)
    n = len(prog.leaves)
    masks = np.zeros((n_rungs, (n + 31) // 32), dtype=np.uint32)
    rows = np.zeros((n_sets, n, 8), dtype=np.uint32)
    for l, leaf in enumerate(prog.leaves):
        for s in range(n_sets):
            v = int.from_bytes(rng.bytes(32), "little") & ((1 << leaf.width) - 1)
            rows[s, l] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
        for r in range(n_rungs):
            if rng.random() < share:
                masks[r, l >> 5] |= np.uint32(1 << (l & 31))
    rung_set = rng.integers(0, n_sets, size=n_rungs).astype(np.uint32)
    rung_set[rng.integers(0, n_rungs)] = n_sets - 1
    return rows, masks, rung_set


def host_fill(case, rows, masks, rung_set, first, lanes, cols=None):
    """The specified SoA of a job: mg_carry_fill_sets_host, which
    tests/test_carry_sets.py holds to mg_carry_fill_rungs_host rung by rung."""
    prog = built(case)[1]
    return E.carry_fill_sets_host(leafgen(case, prog), prog.consts, CASES[case][0], rows, masks,
                                  rung_set, SEED, first, lanes, cols=cols)


@functools.lru_cache(maxsize=None)
def serialized(case):
    cs, prog = built(case)
    return evalref.serialize(cs, prog)


def oracle_result(case, rows, masks, rung_set, first, lanes, cols=None):
    """(first true column or -1, its rung or -1, its rows or None) from the
    oracle on the specified columns."""
    soa = host_fill(case, rows, masks, rung_set, first, lanes, cols)
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
# 1. fill parity
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", (1, 63, 65, 256))
def test_fill_equals_the_host_lane_function(lanes):
    eng = get_engine(0)
    cases, shape = (LADDER, "flats", "rules"), ((3, 2), (1, 1), (4, 3))    # (rungs, sets)
    assert [len(built(c)[1].leaves) for c in cases] == [3, 274, 15]       # padded rows
    pins = [random_sets(c, 11 + k, *shape[k], (0.6, 0.5, 0.5)[k]) for k, c in enumerate(cases)]
    assert pins[1][1][0, 1:].any()                        # pinned leaves past mask bit 31
    assert len(set(pins[2][2].tolist())) > 1              # the rungs of a job read different sets
    res = eng.carry_ladder_sets([(loaded(c),) + p for c, p in zip(cases, pins)], SEED, FIRST,
                                lanes, want_fill=True)
    cols = 4 * lanes
    for c, (rows, masks, rung_set), got in zip(cases, pins, res):
        want = host_fill(c, rows, masks, rung_set, FIRST, lanes, cols)    # the surplus repeats
        assert got[3].shape == want.shape == (len(built(c)[1].leaves), 8, cols)
        assert np.array_equal(got[3], want), (c, lanes)
        # the row set matters: another set on the same rungs fills other words
        if rows.shape[0] > 1:
            other = host_fill(c, rows, masks, (rung_set + 1) % rows.shape[0], FIRST, lanes, cols)
            assert not np.array_equal(other, want)
        # and the returned rows are a column of the region, on the rung reported
        if got[0] >= 0:
            assert np.array_equal(got[2], want[:, :, got[0]])
            assert got[1] == min(got[0] // lanes, masks.shape[0] - 1)
        else:
            assert got[1] == -1 and got[2] is None


# ---------------------------------------------------------------------------
# 2. result parity against the oracle
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ladder_model():
    """Rows of a model of the ladder case, found by the oracle among the
    generator's candidates."""
    n = len(built(LADDER)[1].leaves)
    first, _, rows = oracle_result(LADDER, np.zeros((1, n, 8), dtype=np.uint32),
                                   np.zeros((1, 1), dtype=np.uint32),
                                   np.zeros(1, dtype=np.uint32), 0, 4096)
    assert first >= 0
    return rows


def three_outcomes():
    """(case, rows, masks, rung_set) of: a model in set 0, everything pinned on
    rung 0; a broken row (y >= 2^15) in set 0 and the model in set 1, both
    rungs pinning everything; two sets that both hold the broken y, pinned on
    every rung."""
    prog = built(LADDER)[1]
    names = [l.source for l in prog.leaves]
    model = ladder_model()
    bits = lambda *ns: [sum(1 << names.index(n) for n in ns)]       # noqa: E731
    every = bits(*set(names))
    broken = model.copy()
    broken[names.index("y")] = 0
    broken[names.index("y"), 0] = 0xFFFF
    worse = broken.copy()
    worse[names.index("x")] = 0
    u32 = lambda a: np.array(a, dtype=np.uint32)                    # noqa: E731
    return [(LADDER, u32([model, broken]), u32([every, bits("x"), [0]]), u32([0, 1, 1])),
            (LADDER, u32([broken, model]), u32([every, every]), u32([0, 1])),
            (LADDER, u32([broken, worse]), u32([every, bits("y")]), u32([0, 1]))]


@pytest.mark.parametrize("nreg", (16, 11))
def test_first_rung_and_leaves_equal_the_oracle_on_the_specified_columns(nreg):
    eng = get_engine(0, nreg=nreg)
    jobs = three_outcomes()
    for lanes, first in ((65, 0), (256, FIRST)):
        # the oracle alone: set 0 holds on rung 0; rung 0 misses and rung 1, on set 1, hits
        # in its first column; no rung hits
        want = [oracle_result(c, r, m, s, first, lanes, 3 * lanes) for c, r, m, s in jobs]
        assert want[0][:2] == (0, 0) and np.array_equal(want[0][2], ladder_model())
        assert want[1][:2] == (lanes, 1) and np.array_equal(want[1][2], ladder_model())
        assert want[2] == (-1, -1, None)
        res = eng.carry_ladder_sets([(loaded(c, nreg), r, m, s) for c, r, m, s in jobs], SEED,
                                    first, lanes)
        for g, w in zip(res, want):
            same(g, w)
        # a batch of its own has its own R: the same rung, candidate and rows
        c, r, m, s = jobs[1]
        (alone,) = eng.carry_ladder_sets([(loaded(c, nreg), r, m, s)], SEED, first, lanes)
        same(alone, want[1])
    assert eng.last_kernel_ms() > 0


# ---------------------------------------------------------------------------
# 3. one set is mg_carry_ladder
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", (65, 256))
def test_one_set_is_the_ladder(lanes):
    eng = get_engine(0)
    jobs = []
    for k, (c, n_rungs, share) in enumerate(((LADDER, 3, 0.3), ("rules", 2, 0.5), ("rules", 1, 0.0),
                                             ("flats", 2, 0.5), (LADDER, 4, 0.0))):
        rows, masks, rung_set = random_sets(c, 31 + k, n_rungs, 1, share)
        assert not rung_set.any()
        jobs.append((c, rows, masks, rung_set))
    # and a job that hits: the model's x pinned on rung 1, everything of a broken copy on rung 0
    _, r3, m3, _ = three_outcomes()[0]
    jobs.append((LADDER, r3[1:], m3[:2], np.zeros(2, dtype=np.uint32)))
    res = eng.carry_ladder_sets([(loaded(c), r, m, s) for c, r, m, s in jobs], SEED, FIRST, lanes,
                                want_fill=True)
    old = eng.carry_ladder([(loaded(c), r[0], m) for c, r, m, _ in jobs], SEED, FIRST, lanes,
                           want_fill=True)
    hits = 0
    for got, want in zip(res, old):
        same(got, want)
        assert np.array_equal(got[3], want[3])
        hits += got[0] >= 0
    assert hits >= 2 and res[-1][1] == 1


# ---------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------

def test_the_job_cap_and_the_refusals():
    eng = get_engine(0)
    args = [(loaded(c), r, m, s) for c, r, m, s in three_outcomes()]
    res = eng.carry_ladder_sets(args, SEED, FIRST, 64)
    assert eng.carry_ladder_sets([], SEED, FIRST, 64) == []
    # 257 jobs: Engine.carry_ladder_sets splits, the raw ABI refuses
    many = (args * 86)[:257]
    got = eng.carry_ladder_sets(many, SEED, FIRST, 64)
    assert len(got) == 257
    for k, g in enumerate(got):
        same(g, res[k % 3])
    ms = eng.last_kernel_ms()
    # wrong shapes never reach the library
    lp, r, m, s = args[0]
    for bad in ((lp, r[0], m, s), (lp, r[:, :2], m, s), (lp, r, m[0], s),
                (lp, np.zeros((9, 3, 8), dtype=np.uint32), m, s),
                (lp, np.zeros((0, 3, 8), dtype=np.uint32), m, s),
                (lp, r, np.zeros((9, 1), dtype=np.uint32), np.zeros(9, dtype=np.uint32)),
                (lp, r, np.zeros((3, 2), dtype=np.uint32), s), (lp, r, m, s[:2]),
                (lp, r, m, np.array([0, 1, 2], dtype=np.uint32))):
        with pytest.raises(ValueError):
            eng.carry_ladder_sets([bad], SEED, FIRST, 64)

    def raw(n_jobs, lanes, max_leaves, handles=None, rows=True, masks=True, sets=True, first=True,
            rung=True, out=True, gen=True, jobs_ptr=True, n_rungs=None, n_sets=None,
            rung_set=None):
        arr = (E.CarrySetsJob * max(1, n_jobs))()
        keep = []
        for i in range(n_jobs):
            lp, r, m, s = many[i]
            if rung_set is not None and rung_set[i] is not None:
                s = np.array(rung_set[i], dtype=np.uint32)
                keep.append(s)
            arr[i].prog = handles[i] if handles else lp.handle
            arr[i].pin_rows = E._ptr(r) if rows else None
            arr[i].pin_masks = E._ptr(m) if masks else None
            arr[i].rung_set = E._ptr(s) if sets else None
            arr[i].n_rungs = m.shape[0] if n_rungs is None else n_rungs[i]
            arr[i].n_sets = r.shape[0] if n_sets is None else n_sets[i]
        f = np.zeros(max(1, n_jobs), dtype=np.int64)
        q = np.zeros(max(1, n_jobs), dtype=np.int64)
        o = np.zeros((max(1, n_jobs), max(1, min(max_leaves, 8)), 8), dtype=np.uint32)
        g = Gen(SEED, FIRST)
        rc = eng.lib.mg_carry_ladder_sets(eng._ctx, arr if jobs_ptr else None, n_jobs,
                                          C.byref(g) if gen else None, lanes,
                                          E._ptr(f) if first else None,
                                          E._ptr(q) if rung else None, E._ptr(o) if out else None,
                                          max_leaves, None)
        return rc, eng.lib.mg_last_error(eng._ctx)

    # what mg_carry_ladder refuses
    assert raw(257, 64, 3) == (-1, b"carry_sets: 257 jobs outside 1..256")
    assert raw(0, 64, 3) == (-1, b"carry_sets: 0 jobs outside 1..256")
    assert raw(2, 0, 3) == (-1, b"carry_sets: 0 lanes outside 1..1048576")
    assert raw(2, (1 << 20) + 1, 3) == (-1, b"carry_sets: 1048577 lanes outside 1..1048576")
    for kw in ({"first": False}, {"rung": False}, {"out": False}, {"gen": False},
               {"jobs_ptr": False}):
        assert raw(2, 64, 3, **kw) == (-1, b"carry_sets: null argument")
    assert raw(2, 64, 3, rows=False) == (-1, b"carry_sets: job 0: null pin rows or pin masks")
    assert raw(2, 64, 3, masks=False) == (-1, b"carry_sets: job 0: null pin rows or pin masks")
    assert raw(2, 64, 3, handles=[many[0][0].handle, None]) == \
        (-1, b"carry_sets: job 1: null program")
    other = loaded(LADDER, 11)                          # a program of the 11-slot context
    assert raw(2, 64, 3, handles=[many[0][0].handle, other.handle]) == \
        (-1, b"carry_sets: job 1: a program of another context")
    assert raw(2, 64, 2) == (-1, b"carry_sets: job 0: 3 leaves above max_leaves 2")
    rc, why = raw(2, 64, (1 << 20) + 1)
    assert rc == -1 and why.startswith(b"carry_sets: max_leaves")
    assert raw(2, 64, 3, n_rungs=[3, 0]) == (-1, b"carry_sets: job 1: 0 rungs outside 1..8")
    assert raw(2, 64, 3, n_rungs=[9, 2]) == (-1, b"carry_sets: job 0: 9 rungs outside 1..8")
    assert raw(3, (1 << 20) // 3 + 1, 3) == \
        (-1, b"carry_sets: 3 rungs of 349526 lanes above 1048576 columns")
    # its own: n_sets outside 1..8, a null rung_set, a rung_set entry not below n_sets
    assert raw(2, 64, 3, n_sets=[2, 0]) == (-1, b"carry_sets: job 1: 0 sets outside 1..8")
    assert raw(2, 64, 3, n_sets=[9, 2]) == (-1, b"carry_sets: job 0: 9 sets outside 1..8")
    assert raw(2, 64, 3, sets=False) == (-1, b"carry_sets: job 0: null rung_set")
    assert raw(2, 64, 3, rung_set=[None, [0, 2]]) == \
        (-1, b"carry_sets: job 1: a rung_set entry not below its 2 sets")
    assert raw(2, 64, 3, rung_set=[[0, 1, 0xFFFFFFFF], None]) == \
        (-1, b"carry_sets: job 0: a rung_set entry not below its 2 sets")
    assert raw(2, 64, 3, n_sets=[1, 2]) == \
        (-1, b"carry_sets: job 0: a rung_set entry not below its 1 sets")
    # 256 jobs of 274 leaves at 2^17 lanes x 8 rungs: above the buffer the call may take
    flats = loaded("flats")
    r, m, s = random_sets("flats", 1, 8, 2, 0.5)
    with pytest.raises(E.EngineError, match="bytes needed for 256 jobs"):
        eng.carry_ladder_sets([(flats, r, m, s)] * 256, SEED, 0, 1 << 17)
    assert eng.last_kernel_ms() == ms                   # nothing was launched
    # and the context is still usable
    again = eng.carry_ladder_sets(args, SEED, FIRST, 64)
    for a, b in zip(res, again):
        same(a, b)


# ---------------------------------------------------------------------------
# 5. end to end: the witness that carries is the one carry.union skips
# ---------------------------------------------------------------------------

BVV = symbol_factory.BitVecVal
BVS = symbol_factory.BitVecSym


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


def test_the_second_remembered_witness_carries_the_child_the_first_one_misses(knob):
    x, y, z = (BVS("sets_" + n, 256) for n in "xyz")
    c1, c2, c3, c4 = UGT(x, BVV(5, 256)), UGT(y, x), ULT(z, x), x == BVV(9, 256)
    child = [c1, c2, c3, c4]
    (nodes,) = M.dependence_buckets(M._raw_nodes(child))       # one group: x ties them
    key = lambda cs: M._group_key(M._raw_nodes(cs))            # noqa: E731
    s1, s2 = key([c1, c2]), key([c1, c3])
    w1 = Assignment(vars={"sets_x": 7, "sets_y": 8})
    w2 = Assignment(vars={"sets_x": 9, "sets_z": 1})
    for cs, w in (([c1, c2], w1), ([c1, c3], w2)):            # each a witness of its group
        assert R.eval_constraints([c.raw for c in cs], R.Assignment(w.vars, {}, {})) == 1
    s = M.stats
    models = {}
    for value in ("ladder", "sets"):
        knob(value)
        M._note_hit(s2, w2)                                    # S2 first,
        M._note_hit(s1, w1)                                    # S1 after it: the newest of equals
        assert M._hit_memo.subsets(key(child)) == [s1, s2]
        kind, asg, taken = CY.plan(key(child), M._hit_memo)
        assert (kind, asg.vars, taken) == ("extend", w1.vars, [s1])        # S2 shares x: skipped
        alts = CY.plan_sets(key(child), M._hit_memo)[1]
        assert [(a.vars, t) for a, t in alts] == [(w1.vars, [s1]), (w2.vars, [s2])]
        if value == "sets":
            # on the CPU, by the host fill and the oracle alone: no column of a rung of
            # alternative 0 holds (x pinned to 7 fails x == 9; with x free, y = 8 stays pinned
            # and fails y > 9), and rung "all" of alternative 1 has one within CARRY_LANES
            prog = CY.compile_eval_ck(nodes, alts[0][0], CY.sizes_sets(nodes, alts))
            rows, masks, rung_set, kept = CY.rungs_sets(prog, alts, nodes)
            assert kept[:2] == [(0, 0), (0, 1)] and (2, 0) in kept
            L = CY.CARRY_LANES
            soa = E.carry_fill_sets_host(M.search_leafgen(prog), prog.consts, 0, rows, masks,
                                         rung_set, M.SEARCH_SEED, 0, L)
            ok = evalref.run_leaves_soa(evalref.serialize(nodes, prog), prog, soa)
            for i, (r, a) in enumerate(kept):
                if a == 0:
                    assert not ok[i * L:(i + 1) * L].any(), CY.RUNG_NAMES[r]
            assert ok[L:2 * L].any() and L <= np.flatnonzero(ok)[0] < 2 * L
            # and alternative 0's ladder alone is what knob 2 runs
            r0, m0 = CY.rungs(prog, alts[0][0], *CY.split_nodes(nodes, alts[0][1]))
            soa0 = E.carry_fill_rungs_host(M.search_leafgen(prog), prog.consts, 0, r0, m0,
                                           M.SEARCH_SEED, 0, L)
            assert m0.shape[0] == 2                            # "all" and "new"; "read" repeats
            assert not evalref.run_leaves_soa(evalref.serialize(nodes, prog), prog, soa0).any()
        a = model_of(child)
        models[value] = a
        assert a.vars["sets_x"] == 9 and a.vars["sets_y"] > 9 and a.vars["sets_z"] < 9
        assert s.refuted == 0                                  # the host refutation did not fire
        if value == "ladder":
            # knob 2: S1's witness on every rung, a miss, and the model comes from the search
            assert (s.carry_attempts, s.carry_hits) == (1, 0)
            assert s.carry_rung_hits == [0, 0, 0] and not any(s.carry_set_hits)
            assert search_key(child) in M._SEARCH_CACHE
        else:
            # knob 4: S2's witness on rung "all", and no solve-mode compile of the child
            assert (s.carry_attempts, s.carry_hits) == (1, 1)
            assert s.carry_rung_hits == [1, 0, 0] and s.carry_set_hits[:2] == [0, 1]
            assert sum(s.carry_set_hits) == 1
            assert search_key(child) not in (M._SEARCH_CACHE or {})   # (nothing was searched)
            assert a.vars["sets_z"] == 1                      # the remembered value, kept
            assert "rung hits: 1/0/0 set hits: 0/1/0/0" in repr(s)


# ---------------------------------------------------------------------------
# 6. streams, knob 4 against knob off
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
def test_streams_lose_no_model_and_gain_no_wrong_one_under_the_sets(knob, stream):
    qs = W.queries(stream, LABELS["n"])[:64]
    unsat = {r["i"] for r in LABELS["streams"].get(stream, ()) if r["label"] == "unsat"}
    knob(False)
    off = run_stream(qs)
    knob("sets")
    on = run_stream(qs)
    s = M.stats
    print("sets %s: models off %d on %d; exact %d attempts %d hits %d rungs %s sets %s gated %d" % (
        stream, sum(a is not None for a in off), sum(a is not None for a in on), s.carry_exact,
        s.carry_attempts, s.carry_hits, s.carry_rung_hits, s.carry_set_hits, s.carry_gated))
    for i, (q, a, b) in enumerate(zip(qs, off, on)):
        if a is not None:
            assert b is not None, (stream, i)
        if b is not None:
            assert R.eval_constraints(list(q), R.Assignment(b.vars, b.arrays, b.funcs)) == 1, \
                (stream, i)
            assert i not in unsat, (stream, i)
    assert s.carry_exact > 0

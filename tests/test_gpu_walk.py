"""The scored walk on the GPU (mg_walk, csrc/mg_walk.hip):
Engine.walk against walk_ref through the oracle (oracle/evalref.c) in every
output on the crafted cases (tests/walk_cases.py), on both register layouts,
at lane counts around the wave and block sizes and at 1, 2, 3 and 64 walkers;
one flat walker against Engine.repair; determinism; a start that is a model;
the sync interval; the refusals of the C ABI; repair_group(scored=True) on the
crafted cases, every model checked by oracle/smtlib_ref.py; and
MYTHRIL_GPU_REPAIR=2 through get_model."""

import ctypes as C

import numpy as np
import pytest

import repair_cases as RK
import walk_cases as K
from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import EngineError, default_leafgen, get_engine
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N

pytestmark = pytest.mark.gpu

SHORT = 8             # rounds at the shapes below the cases' own
# (lanes, walkers) at SHORT rounds; 64 walkers: at most 256 lanes
PLAN = ((1, 1), (1, 3), (63, 2), (64, 3), (65, 1), (256, 64), (1000, 2), (4096, 2))


def loaded(name, nreg=16):
    """(engine of the layout, the case's eval-form program with mask and
    residual probes loaded with the default generator, root count, table,
    residual count)."""
    prog = K.program(name, nreg)
    ref = K.program(name)                        # the reference ran on this program's tables
    assert prog.const_values == ref.const_values and len(prog.leaves) == len(ref.leaves)
    probes, table = K.scoring(name)
    n_roots = len(K.case(name)[0])
    assert prog.n_probes == CS.n_mask_probes(n_roots) + len(probes)
    eng = get_engine(0, nreg=nreg)
    return eng, eng.load(prog, default_leafgen(prog), prog_seed=0), n_roots, table, len(probes)


def same(got, want, rounds_too=True):
    assert np.array_equal(got.leaves, want.leaves)
    assert np.array_equal(got.nfail, want.nfail) and np.array_equal(got.cost, want.cost)
    assert got.winner == want.winner
    if rounds_too:
        assert got.rounds == want.rounds
        assert np.array_equal(got.trace, want.trace)


@pytest.mark.parametrize("nreg", (16, 11))
@pytest.mark.parametrize("name", K.NAMES)
def test_walk_equals_the_reference(name, nreg):
    eng, lp, n_roots, table, n_resid = loaded(name, nreg)
    assert eng.nreg == nreg
    for lanes, walkers in PLAN:
        got = eng.walk(lp, K.starts(name, walkers), n_roots, table, n_resid, K.SEED, lanes, SHORT)
        want = K.reference(name, walkers, lanes, SHORT)
        assert got.trace.shape == (walkers, SHORT, 2) and got.leaves.shape == want.leaves.shape
        same(got, want)
        if lanes == 1:          # the start, with its own key, after every round
            assert np.array_equal(got.leaves, K.starts(name, walkers)) and got.rounds == SHORT
            assert (got.nfail > 0).all() and (got.cost >= got.nfail).all() and got.winner == 0
            assert (got.trace[:, :, 0] == got.nfail[:, None]).all()
    got = eng.walk(lp, K.starts(name, 1), n_roots, table, n_resid, K.SEED, K.LANES,
                   K.MAX_ROUNDS[name])
    same(got, K.reference(name))
    assert got.nfail[0] == 0 and got.rounds <= K.MAX_ROUNDS[name] // 2 and got.kernel_ms > 0


@pytest.mark.parametrize("name", ("narrow", "twins"))
def test_one_flat_walker_equals_repair(name):
    prog = RK.masked_program(name)
    eng = get_engine(0, nreg=16)
    lp = eng.load(prog, default_leafgen(prog), prog_seed=0)
    n_roots = len(RK.case(name)[0])
    start = RK.start_rows(name)
    for lanes, rounds in ((1000, 24), (RK.LANES, RK.MAX_ROUNDS)):
        rep = eng.repair(lp, start, n_roots, RK.SEED, lanes, rounds)
        got = eng.walk(lp, start[None], n_roots, RP.flat_table(n_roots), 0, RK.SEED, lanes, rounds)
        assert np.array_equal(got.leaves[0], rep.leaves) and got.winner == 0
        assert int(got.nfail[0]) == rep.nfail == int(got.cost[0]) and got.rounds == rep.rounds
        assert np.array_equal(got.trace[0, :, 0], rep.trace)
        assert np.array_equal(got.trace[0, :, 1], rep.trace)


def test_two_runs_are_bit_identical():
    eng, lp, n_roots, table, n_resid = loaded("mixed")
    args = (lp, K.starts("mixed", 3), n_roots, table, n_resid)
    a = eng.walk(*args, K.SEED, 1000, SHORT)
    b = eng.walk(*args, K.SEED, 1000, SHORT)
    same(a, b)
    other = eng.walk(*args, K.SEED + 1, 1000, SHORT)
    assert not np.array_equal(other.trace, a.trace) or not np.array_equal(other.leaves, a.leaves)


@pytest.mark.parametrize("name", K.NAMES)
def test_a_satisfying_start_returns_itself(name):
    eng, lp, n_roots, table, n_resid = loaded(name)
    model = np.array(K.reference(name).leaves[0])
    starts = np.stack([K.start_rows(name), model])           # walker 1 starts at a model
    for sync in (1, 8):
        got = eng.walk(lp, starts, n_roots, table, n_resid, K.SEED, 256, K.MAX_ROUNDS[name], sync)
        assert np.array_equal(got.leaves[1], model) and got.nfail[1] == 0 == got.cost[1]
        assert got.rounds == sync and not got.trace[1].any() and got.winner == 1


@pytest.mark.parametrize("name", ("magnitude", "mixed"))
def test_sync_interval_only_delays_the_stop(name):
    eng, lp, n_roots, table, n_resid = loaded(name)
    rounds = K.MAX_ROUNDS[name]
    runs = [eng.walk(lp, K.starts(name, 1), n_roots, table, n_resid, K.SEED, K.LANES, rounds, s)
            for s in (1, 8, rounds)]
    same(runs[1], K.reference(name))
    a, b, c = runs
    assert a.nfail[0] == b.nfail[0] == c.nfail[0] == 0
    assert np.array_equal(a.leaves, b.leaves) and np.array_equal(b.leaves, c.leaves)
    assert a.rounds <= b.rounds <= c.rounds == rounds and b.rounds % 8 == 0
    assert a.rounds == K.FIRST_ZERO[name] + 1
    assert np.array_equal(a.trace[:, :a.rounds], b.trace[:, :a.rounds])
    assert np.array_equal(b.trace[:, :b.rounds], c.trace[:, :b.rounds])


def test_refusals_launch_nothing_and_leave_the_context_usable():
    name = "mixed"
    eng, lp, n_roots, table, n_resid = loaded(name)
    starts = K.starts(name, 2)
    good = eng.walk(lp, starts, n_roots, table, n_resid, K.SEED, 256, SHORT)
    ms = eng.last_kernel_ms()
    assert ms > 0
    unknown, beyond = np.array(table), np.array(table)
    unknown[5] = 3 << 16
    beyond[256] = RP.MAGNITUDE << 16 | n_resid
    bad = [dict(starts=K.starts(name, 65)), dict(starts=starts[:0]), dict(n_roots=0),
           dict(n_roots=1025), dict(mask_probe0=1), dict(mask_probe0=5), dict(lanes=0),
           dict(lanes=(1 << 20) + 1), dict(max_rounds=0), dict(max_rounds=(1 << 16) + 1),
           dict(table=unknown), dict(table=beyond), dict(n_resid=n_resid + 1)]
    for kw in bad:
        args = dict(starts=starts, n_roots=n_roots, table=table, n_resid=n_resid, seed=K.SEED,
                    lanes=256, max_rounds=SHORT)
        args.update(kw)
        with pytest.raises(EngineError, match=r"\(-1\): .*walk"):
            eng.walk(lp, **args)
        assert eng.last_kernel_ms() == ms, kw             # no launch was timed
    # probes that would need more than 256 MiB
    x = N.bv_var("x", 256)
    cs = [N.eq(N.extract(7, 0, x), N.bv_num(3, 8))]
    many = compile_constraints(cs, CS.mask_probes(cs) + [N.extract(8 * i + 7, 8 * i, x)
                                                         for i in range(1, 10)])
    assert many.n_probes == 10
    lp_many = eng.load(many, default_leafgen(many), prog_seed=0)
    zero = np.zeros((64, 1, 8), dtype=np.uint32)
    flat = RP.flat_table(1)
    with pytest.raises(EngineError, match=r"\(-1\): .*census view"):
        eng.walk(lp_many, zero, 1, flat, 0, K.SEED, 1 << 14, SHORT)
    assert eng.last_kernel_ms() == ms
    assert eng.walk(lp_many, zero[:2], 1, flat, 0, K.SEED, 1 << 10, SHORT).rounds == SHORT
    ms = eng.last_kernel_ms()
    # a program with no leaves
    cs = [N.eq(N.bv_num(1, 8), N.bv_num(1, 8))]
    ground = compile_constraints(cs, CS.mask_probes(cs))
    assert len(ground.leaves) == 0 and ground.n_probes == 1
    lp_ground = eng.load(ground, default_leafgen(ground), prog_seed=0)
    with pytest.raises(EngineError, match=r"\(-1\): .*no leaves"):
        eng.walk(lp_ground, np.zeros((1, 0, 8), dtype=np.uint32), 1, flat, 0, K.SEED, 64, SHORT)
    # null pointers (trace may be null)
    out = np.zeros_like(starts)
    nf, co = np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    nr, win = C.c_uint32(), C.c_uint32()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    tab = np.ascontiguousarray(table)
    full = [eng._ctx, lp.handle, p(starts), 2, n_roots, 0, p(tab), n_resid, K.SEED, 256, SHORT, 8,
            p(out), p(nf), p(co), C.byref(nr), None, C.byref(win)]
    for k in (1, 2, 6, 12, 13, 14, 15, 17):
        q = list(full)
        q[k] = None
        assert eng.lib.mg_walk(*q) == -1 and b"null" in eng.lib.mg_last_error(eng._ctx)
    assert eng.last_kernel_ms() == ms
    assert eng.lib.mg_walk(*full) == 0
    assert nr.value == good.rounds and win.value == good.winner
    assert np.array_equal(out, good.leaves) and np.array_equal(nf, good.nfail)
    assert np.array_equal(co, good.cost)
    # and the next valid call succeeds
    same(eng.walk(lp, starts, n_roots, table, n_resid, K.SEED, 256, SHORT), good)


def oracle_values(constraints, a):
    from oracle import smtlib_ref as R
    return R.evaluate(list(constraints), R.Assignment(a.vars, a.arrays, a.funcs))


# mixed: the census's best candidate has about half of the 250 bits of x wrong
# (the generator draws them), one or two of which a round repairs
GROUP_ROUNDS = {"mixed": 256}


@pytest.mark.parametrize("name", K.NAMES)
def test_repair_group_scored_solves_what_the_count_cannot(name):
    cs, _ = K.case(name)
    kw = dict(form="eval", max_rounds=GROUP_ROUNDS.get(name, K.MAX_ROUNDS[name]))
    g = RP.repair_group(cs, scored=True, walkers=4, **kw)
    assert g["status"] == RP.REPAIRED, (g["status"], g.get("why"), g.get("repair"))
    assert g["census"].n_sat == 0 and g["start"]["nfail"] > 0        # the generator missed
    res = g["repair"]
    assert len(g["starts"]) == 4 == len(res.nfail) and g["starts"][0] == g["start"]["index"]
    assert res.nfail[res.winner] == 0 and res.rounds <= kw["max_rounds"]
    assert all(oracle_values(cs, g["assignment"]))
    print(name, "starts", g["starts"], "rounds", res.rounds, "winner", res.winner,
          "trace", res.trace[res.winner, :res.rounds].tolist())
    if name != "mixed":
        flat = RP.repair_group(cs, **kw)                             # scored=False: today's path
        assert flat["status"] == RP.STUCK and flat["repair"].nfail > 0
        assert "assignment" not in flat and "starts" not in flat


def gap_query():
    """(u ^ v) - w == 0 over three 64-bit symbols with the guards of the
    crafted cases: the search form's model construction solves a plain
    u ^ v == w outright (compare twins_query of tests/test_gpu_repair.py), and
    no copy plus a boundary value is a model."""
    from mythril_amd.smt import Extract, Not, symbol_factory
    u, v, w = (symbol_factory.BitVecSym("gap_" + s, 64) for s in "uvw")
    val = symbol_factory.BitVecVal
    cons = [(u ^ v) - w == val(0, 64)]
    for s in (u, v, w):
        cons += [Not(Extract(lo + 15, lo, s) == val(k, 16)) for lo in (16, 40) for k in (0, 0xFFFF)]
    return tuple(cons)


@pytest.fixture
def model_state():
    import mythril_amd.model as M
    get_engine(0)                                  # not on the query's budget
    M.get_model.cache_clear()
    M.clear_search_memos()
    M.time_handler.start_execution(3600)
    M.stats.reset_gpu()
    yield M
    M.configure_from_env({})
    M.clear_search_memos()
    M.get_model.cache_clear()
    M.stats.reset_gpu()


def test_get_model_closes_the_gap_with_the_scored_walk(model_state):
    M = model_state
    M.configure_from_env({"MYTHRIL_GPU_REPAIR": "2", "MYTHRIL_GPU_BUDGET_MS": "5000"})
    assert M.REPAIR and M.REPAIR_SCORED
    cons = gap_query()
    try:
        m = M.get_model(cons, enforce_execution_time=False)
    finally:
        M.SEARCH_BUDGET_MS = 200
    assert (M.stats.repair_attempts, M.stats.repair_hits) == (1, 1)
    assert M.stats.gpu_hits == 1 and not M._group_miss
    assert all(oracle_values([c.raw for c in cons], m.assignment))
    assert "GPU repair: attempts: 1 hits: 1" in M.stats.gpu_report()


def test_get_model_misses_the_gap_with_the_count_alone(model_state):
    M = model_state
    M.configure_from_env({"MYTHRIL_GPU_REPAIR": "1", "MYTHRIL_GPU_BUDGET_MS": "5000"})
    assert M.REPAIR and not M.REPAIR_SCORED
    try:                                     # (z3 absent: nothing decides a miss)
        M.get_model(gap_query(), enforce_execution_time=False)
    except M.SolverUnavailable:
        pass
    finally:
        M.SEARCH_BUDGET_MS = 200
    assert (M.stats.repair_attempts, M.stats.repair_hits) == (1, 0)
    assert M.stats.gpu_queries == 1 and M.stats.gpu_hits == 0 and M._group_miss
    M.configure_from_env({"MYTHRIL_GPU_REPAIR": "0"})
    assert not M.REPAIR and not M.REPAIR_SCORED

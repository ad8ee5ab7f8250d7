"""The local search on the GPU (mg_repair, csrc/mg_repair.hip; DESIGN.md
§3.9): Engine.repair against repair_ref through the oracle (oracle/evalref.c)
in every output on the crafted cases (tests/repair_cases.py), on both register
layouts and at lane counts around the wave and block sizes; the sync
interval; determinism; a start that is a model; the refusals of the C ABI;
repair_group on the crafted cases and on stream queries, every model checked
by oracle/smtlib_ref.py; and the MYTHRIL_GPU_REPAIR hook of get_model."""

import ctypes as C

import numpy as np
import pytest

import repair_cases as K
from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import EngineError, default_leafgen, get_engine
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N

pytestmark = pytest.mark.gpu

LANES = (1, 63, 64, 65, 256, 1000, 4096)
SHORT = 24            # rounds at the lane counts below the cases' own 4096


def loaded(name, nreg=16):
    """(engine of the layout, the case's masked eval-form program loaded with
    the default generator, its root count)."""
    prog = K.masked_program(name, nreg)
    ref = K.masked_program(name)                 # the reference ran on this program's tables
    assert prog.const_values == ref.const_values and len(prog.leaves) == len(ref.leaves)
    eng = get_engine(0, nreg=nreg)
    return eng, eng.load(prog, default_leafgen(prog), prog_seed=0), len(K.case(name)[0])


def same(got, want, rounds_too=True):
    assert np.array_equal(got.leaves, want.leaves)
    assert got.nfail == want.nfail
    if rounds_too:
        assert got.rounds == want.rounds
        assert np.array_equal(got.trace, want.trace)


@pytest.mark.parametrize("nreg", (16, 11))
@pytest.mark.parametrize("name", K.NAMES)
def test_repair_equals_the_reference(name, nreg):
    eng, lp, n_roots = loaded(name, nreg)
    assert eng.nreg == nreg
    start = K.start_rows(name)
    for lanes in LANES:
        rounds = K.MAX_ROUNDS if lanes == K.LANES else SHORT
        got = eng.repair(lp, start, n_roots, K.SEED, lanes, rounds)
        want = K.reference(name, lanes, rounds)
        assert got.trace.shape == (rounds,)
        same(got, want)
        if lanes == 1:          # the start, with its own count, after every round
            assert np.array_equal(got.leaves, start) and got.rounds == rounds
            assert got.nfail == int((~K.bits_fn(name)(start[:, :, None])[0]).sum()) > 0
        if lanes == K.LANES:
            assert got.nfail == 0 and got.kernel_ms > 0


@pytest.mark.parametrize("name", ("bytes", "wide"))
def test_sync_interval_only_delays_the_stop(name):
    eng, lp, n_roots = loaded(name)
    start = K.start_rows(name)
    runs = [eng.repair(lp, start, n_roots, K.SEED, K.LANES, K.MAX_ROUNDS, s)
            for s in (1, 8, K.MAX_ROUNDS)]
    for s, r in zip((1, 8, K.MAX_ROUNDS), runs):
        same(r, K.reference(name, K.LANES, K.MAX_ROUNDS, s))
    a, b, c = runs
    assert a.nfail == b.nfail == c.nfail == 0
    assert np.array_equal(a.leaves, b.leaves) and np.array_equal(b.leaves, c.leaves)
    assert a.rounds <= b.rounds <= c.rounds == K.MAX_ROUNDS and b.rounds % 8 == 0
    assert a.trace[a.rounds - 1] == 0 and (a.rounds == 1 or a.trace[a.rounds - 2] > 0)
    assert np.array_equal(a.trace[:a.rounds], b.trace[:a.rounds])
    assert np.array_equal(b.trace[:b.rounds], c.trace[:b.rounds])


def test_two_runs_are_bit_identical():
    eng, lp, n_roots = loaded("narrow")
    start = K.start_rows("narrow")
    a = eng.repair(lp, start, n_roots, K.SEED, 1000, SHORT)
    b = eng.repair(lp, start, n_roots, K.SEED, 1000, SHORT)
    same(a, b)
    other = eng.repair(lp, start, n_roots, K.SEED + 1, 1000, SHORT)
    assert not np.array_equal(other.trace, a.trace) or not np.array_equal(other.leaves, a.leaves)


@pytest.mark.parametrize("name", K.NAMES)
def test_a_satisfying_start_returns_itself(name):
    eng, lp, n_roots = loaded(name)
    model = np.array(K.reference(name).leaves)
    for sync in (1, 8):
        got = eng.repair(lp, model, n_roots, K.SEED, 256, K.MAX_ROUNDS, sync)
        assert np.array_equal(got.leaves, model) and got.nfail == 0
        assert got.rounds == sync and not got.trace.any()


def test_refusals_launch_nothing_and_leave_the_context_usable():
    eng, lp, n_roots = loaded("wide")
    start = K.start_rows("wide")
    good = eng.repair(lp, start, n_roots, K.SEED, 256, 8)
    ms = eng.last_kernel_ms()
    assert ms > 0
    bad = [dict(n_roots=0), dict(n_roots=1025), dict(n_roots=513), dict(mask_probe0=1),
           dict(mask_probe0=2), dict(lanes=0), dict(lanes=(1 << 20) + 1), dict(max_rounds=0),
           dict(max_rounds=(1 << 16) + 1)]
    for kw in bad:
        args = dict(n_roots=n_roots, seed=K.SEED, lanes=256, max_rounds=8)
        args.update(kw)
        with pytest.raises(EngineError, match=r"\(-1\): .*repair"):
            eng.repair(lp, start, **args)
        assert eng.last_kernel_ms() == ms, kw             # no launch was timed
    # a program whose probes would need more than 256 MiB
    x = N.bv_var("x", 256)
    cs = [N.eq(N.extract(7, 0, x), N.bv_num(3, 8))]
    many = compile_constraints(cs, CS.mask_probes(cs) + [N.extract(8 * i + 7, 8 * i, x)
                                                         for i in range(1, 10)])
    assert many.n_probes == 10
    lp_many = eng.load(many, default_leafgen(many), prog_seed=0)
    zero = np.zeros((1, 8), dtype=np.uint32)
    with pytest.raises(EngineError, match=r"\(-1\): .*census view"):
        eng.repair(lp_many, zero, 1, K.SEED, 1 << 20, 8)
    assert eng.repair(lp_many, zero, 1, K.SEED, 1 << 10, 8).rounds == 8
    ms = eng.last_kernel_ms()
    # a program with no leaves
    cs = [N.eq(N.bv_num(1, 8), N.bv_num(1, 8))]
    ground = compile_constraints(cs, CS.mask_probes(cs))
    assert len(ground.leaves) == 0 and ground.n_probes == 1
    lp_ground = eng.load(ground, default_leafgen(ground), prog_seed=0)
    with pytest.raises(EngineError, match=r"\(-1\): .*no leaves"):
        eng.repair(lp_ground, np.zeros((0, 8), dtype=np.uint32), 1, K.SEED, 64, 8)
    # null pointers (trace may be null)
    out = np.zeros_like(start)
    nf, nr = C.c_uint32(), C.c_uint32()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    full = [eng._ctx, lp.handle, p(start), n_roots, 0, K.SEED, 256, 8, 8, p(out), C.byref(nf),
            C.byref(nr), None]
    for k in (1, 2, 9, 10, 11):
        q = list(full)
        q[k] = None
        assert eng.lib.mg_repair(*q) == -1 and b"null" in eng.lib.mg_last_error(eng._ctx)
    assert eng.last_kernel_ms() == ms
    assert eng.lib.mg_repair(*full) == 0
    assert (nf.value, nr.value) == (good.nfail, good.rounds) and np.array_equal(out, good.leaves)
    # and the next valid call succeeds
    same(eng.repair(lp, start, n_roots, K.SEED, 256, 8), good)


def oracle_values(constraints, a):
    from oracle import smtlib_ref as R
    return R.evaluate(list(constraints), R.Assignment(a.vars, a.arrays, a.funcs))


# step: a walker at the census's best candidate (only y - x == 1 fails) needs
# y := x and y += 1 in ONE lane, once in 147456 two-move lanes
GROUP_KW = {"step": dict(lanes=1 << 18, max_rounds=16)}


@pytest.mark.parametrize("name", K.NAMES)
def test_repair_group_solves_the_crafted_cases(name):
    cs, _ = K.case(name)
    g = RP.repair_group(cs, form="eval", **GROUP_KW.get(name, {}))
    assert g["status"] == RP.REPAIRED, (g["status"], g.get("why"), g.get("repair"))
    assert g["census"].n_sat == 0 and g["start"]["nfail"] > 0        # the generator missed
    assert g["repair"].nfail == 0 and g["repair"].rounds <= 64
    assert all(oracle_values(cs, g["assignment"]))
    print(name, "start", g["start"], "rounds", g["repair"].rounds,
          "trace", g["repair"].trace[:g["repair"].rounds].tolist())


def stream_query(wl, qi):
    """Query ``qi`` of a stream as the recall labels index it."""
    import json
    import os
    from mythril_amd import workloads as W
    here = os.path.dirname(os.path.abspath(__file__))
    n = json.load(open(os.path.join(here, "golden", "recall_labels.json")))["n"]
    return W.queries(wl, n)[qi]


@pytest.mark.parametrize("qi", range(8))
@pytest.mark.parametrize("wl", ("c4", "c3o"))
def test_stream_models_pass_the_oracle_and_refuted_groups_get_none(wl, qi):
    import mythril_amd.model as M
    from mythril_amd.refute import refuted
    known = {RP.REPAIRED, RP.STUCK, CS.REFUTED, CS.GROUND_TRUE, CS.GROUND_FALSE, CS.DEAD,
             CS.UNSUPPORTED}
    for group in M.dependence_buckets(stream_query(wl, qi)):
        g = RP.repair_group(group, form="search")
        assert g["status"] in known
        if len(group) > 1 and refuted(group):
            assert g["status"] == CS.REFUTED
        if g["status"] != RP.REPAIRED:
            assert "assignment" not in g
            continue
        assert all(oracle_values(group, g["assignment"]))


def twins_query():
    """Crafted case (ii) through mythril_amd.smt.  The equality is written
    x - y == 0: the search form's model construction solves a plain x == y
    outright (y := x), which leaves nothing to repair."""
    from mythril_amd.smt import Extract, Not, symbol_factory
    x, y = symbol_factory.BitVecSym("tw_x", 256), symbol_factory.BitVecSym("tw_y", 256)
    val = symbol_factory.BitVecVal
    a, b = Extract(79, 64, x), Extract(143, 128, x)
    return tuple([x - y == val(0, 256), Not(x == val(0, 256))] +
                 [Not(w == val(v, 16)) for w in (a, b) for v in (0, 0xFFFF)])


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


def test_get_model_repairs_a_miss_when_asked(model_state):
    M = model_state
    M.configure_from_env({"MYTHRIL_GPU_REPAIR": "1", "MYTHRIL_GPU_BUDGET_MS": "5000"})
    assert M.REPAIR
    cons = twins_query()
    try:
        m = M.get_model(cons, enforce_execution_time=False)
    finally:
        M.SEARCH_BUDGET_MS = 200
    assert (M.stats.repair_attempts, M.stats.repair_hits) == (1, 1)
    assert M.stats.gpu_hits == 1 and not M._group_miss
    assert all(oracle_values([c.raw for c in cons], m.assignment))
    assert "GPU repair: attempts: 1 hits: 1" in M.stats.gpu_report()
    M.stats.reset_gpu()
    assert (M.stats.repair_attempts, M.stats.repair_hits) == (0, 0)


def test_get_model_does_not_repair_unasked(model_state):
    M = model_state
    M.configure_from_env({})
    assert not M.REPAIR
    blank = M.stats.gpu_report()
    assert "repair" not in blank and "repair" not in repr(M.stats)
    try:                                     # (z3 absent: nothing decides a miss)
        M.get_model(twins_query(), enforce_execution_time=False)
    except M.SolverUnavailable:
        pass
    assert (M.stats.repair_attempts, M.stats.repair_hits) == (0, 0)
    assert "repair" not in M.stats.gpu_report()
    assert M.stats.gpu_queries == 1 and M.stats.gpu_hits == 0 and M._group_miss
    M.stats.reset_gpu()
    assert M.stats.gpu_report() == blank

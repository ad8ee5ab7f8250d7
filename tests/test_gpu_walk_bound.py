"""The walk with aims for orders on the GPU (mg_walk_bound,
csrc/mg_walk_bound.hip): Engine.walk_bound against walk_ref
with the tree scoring and the table through the oracle (oracle/evalref.c) in
every output on the crafted cases (tests/bound_cases.py), on both register
layouts, at lane counts around the wave and block sizes, below the live list's
length and at 1, 2, 3 and 64 walkers; on the generated cases of
tests/gen_cases.py whose truth bits lie past one mask word and one mask probe;
a table of XOR entries against Engine.walk_aim and an empty one against
Engine.walk_tree; determinism; the refusals of the C ABI;
repair_group(scored="bound") on the crafted cases, every model checked by
oracle/smtlib_ref.py; and MYTHRIL_GPU_REPAIR=5 through get_model."""

import ctypes as C
import functools

import numpy as np
import pytest

import aim_cases as AC
import bound_cases as BC
import gen_cases as GC
import tree_cases as K
from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import EngineError, default_leafgen, get_engine

pytestmark = pytest.mark.gpu

SHORT = 8             # rounds at the shapes below the cases' own
# (lanes, walkers) at SHORT rounds; 64 walkers: at most 256 lanes; 16 and 24
# lanes: cap = 2 and 3 live lanes, at or below the live entries of a case
PLAN = ((1, 1), (1, 3), (16, 2), (24, 1), (63, 2), (64, 3), (65, 1), (256, 64), (1000, 2),
        (4096, 2))


def loaded(name, nreg=16, cases=BC):
    """(engine of the layout, the case's eval-form program with root mask,
    atom mask and residual probes loaded with the default generator, root
    count, trees)."""
    prog = cases.program(name, nreg)
    ref = cases.program(name)                    # the reference ran on this program's tables
    assert prog.const_values == ref.const_values
    assert [(l.kind, l.source, l.chunk, l.width) for l in prog.leaves] == \
        [(l.kind, l.source, l.chunk, l.width) for l in ref.leaves]      # the table's leaves
    T = cases.trees(name)
    cs = cases.case(name)
    n_roots = len(cs[0] if isinstance(cs, tuple) else cs)
    assert prog.n_probes == (CS.n_mask_probes(n_roots) + CS.n_mask_probes(T.n_atoms)
                             + T.n_resid)
    eng = get_engine(0, nreg=nreg)
    return eng, eng.load(prog, default_leafgen(prog), prog_seed=0), n_roots, T


def same(got, want):
    assert np.array_equal(got.leaves, want.leaves)
    assert np.array_equal(got.nfail, want.nfail) and np.array_equal(got.cost, want.cost)
    assert got.winner == want.winner and got.rounds == want.rounds
    assert np.array_equal(got.trace, want.trace)


@pytest.mark.parametrize("nreg", (16, 11))
@pytest.mark.parametrize("name", BC.NAMES)
def test_walk_bound_equals_the_reference(name, nreg):
    eng, lp, n_roots, T = loaded(name, nreg)
    assert eng.nreg == nreg
    B = BC.bounds(name)
    assert B.n_order == len(B) >= 2
    for lanes, walkers in PLAN:
        got = eng.walk_bound(lp, BC.starts(name, walkers), n_roots, T, B, BC.SEED, lanes, SHORT)
        want = BC.reference(name, walkers, lanes, SHORT)
        assert got.trace.shape == (walkers, SHORT, 2) and got.leaves.shape == want.leaves.shape
        same(got, want)
        if lanes == 1:          # the start, with its own key, after every round
            assert np.array_equal(got.leaves, BC.starts(name, walkers)) and got.rounds == SHORT
            assert (got.nfail == 1).all() and got.winner == 0
    got = eng.walk_bound(lp, BC.starts(name, 1), n_roots, T, B, BC.SEED, BC.LANES,
                         BC.MAX_ROUNDS[name])
    same(got, BC.reference(name))
    assert got.nfail[0] == 0 and got.rounds <= BC.MAX_ROUNDS[name] // 2 and got.kernel_ms > 0


# ---------------------------------------------------------------------------
# the generated cases: truth bits past one mask word and one mask probe
# ---------------------------------------------------------------------------

GEN_SHAPES = GC.SHAPES[:2] + ((16, 2),)


@functools.lru_cache(maxsize=None)
def gen_bounds(name):
    B = RP.bound_table(GC.case(name), GC.trees(name), GC.program(name))
    for a in (B.entries, B.pieces, B.fixed):
        a.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def gen_reference(name, walkers, lanes):
    prog, T = GC.program(name), GC.trees(name)
    return RP.walk_ref(GC.values_fn(name), default_leafgen(prog), GC.consts_of(prog),
                       GC.starts(name, walkers), T.roots, GC.SEED, lanes, GC.ROUNDS, 8,
                       score=RP.tree_scoring(T), bounds=gen_bounds(name))


def test_the_generated_tables_reach_past_a_mask_word_and_a_mask_probe():
    B = gen_bounds("rules")
    truth = [int(t) for t in B.entries[B.entries[:, 3] != RP.BOUND_XOR, 4]]
    atoms = [t & ~RP.BOUND_ATOM for t in truth if t & RP.BOUND_ATOM]
    assert atoms and max(atoms) >= 32 and any(not t & RP.BOUND_ATOM for t in truth)
    B = gen_bounds("ladder_lt")
    assert len(B) == RP.AIM_MAX_ENTRIES == 256           # the cap: 1 XOR entry, 256 orders
    assert len(GC.aims("ladder_lt")) == 1 and B.n_order == 255
    assert [int(t) for t in B.entries[1:, 4]] == list(range(255))     # the first ones
    assert (B.entries[1:, 3] == RP.BOUND_LOW_STRICT).all()


@pytest.mark.parametrize("nreg", (16, 11))
@pytest.mark.parametrize("name", ("rules", "ladder_lt"))
def test_generated_cases_equal_the_reference(name, nreg):
    eng, lp, n_roots, T = loaded(name, nreg, GC)         # (both compile on both layouts)
    B = gen_bounds(name)
    adopted = 0
    for lanes, walkers in GEN_SHAPES:
        got = eng.walk_bound(lp, GC.starts(name, walkers), n_roots, T, B, GC.SEED, lanes,
                             GC.ROUNDS)
        want = gen_reference(name, walkers, lanes)
        same(got, want)
        tree = GC.reference(name, walkers, lanes)
        adopted += not np.array_equal(want.trace, tree.trace)
    assert adopted                                       # the order entries changed the walk


# ---------------------------------------------------------------------------
# narrower tables
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", AC.NAMES)
def test_xor_entries_alone_are_walk_aim_bit_for_bit(name):
    eng, lp, n_roots, T = loaded(name, 16, AC)
    A = AC.aims(name)
    B = RP.bounds_of_aims(A, n_roots, T.n_atoms)
    assert len(B) == len(A) and B.n_order == 0
    for lanes, walkers in ((16, 2), (64, 3), (1000, 2)):
        starts = AC.starts(name, walkers)
        want = eng.walk_aim(lp, starts, n_roots, T, A, AC.SEED, lanes, SHORT)
        same(eng.walk_bound(lp, starts, n_roots, T, B, AC.SEED, lanes, SHORT), want)
        if (lanes, walkers) != (16, 2):
            same(want, AC.reference(name, walkers, lanes, SHORT))


@pytest.mark.parametrize("name", K.NAMES)
def test_an_empty_table_is_walk_tree_bit_for_bit(name):
    eng, lp, n_roots, T = loaded(name, 16, K)
    for lanes, walkers in ((64, 3), (1000, 2)):
        starts = K.starts(name, walkers)
        want = eng.walk_tree(lp, starts, n_roots, T, K.SEED, lanes, 16)
        same(eng.walk_bound(lp, starts, n_roots, T, RP.make_bounds([]), K.SEED, lanes, 16), want)
        same(want, K.reference(name, walkers, lanes, 16))


def test_two_runs_are_identical_and_another_seed_differs():
    name = "signed"
    eng, lp, n_roots, T = loaded(name)
    B = BC.bounds(name)
    run = lambda seed: eng.walk_bound(lp, BC.starts(name, 3), n_roots, T, B, seed, 1000, SHORT)
    a, b, c = run(BC.SEED), run(BC.SEED), run(BC.SEED + 1)
    same(a, b)
    assert not np.array_equal(a.leaves, c.leaves)
    same(c, BC.reference(name, 3, 1000, SHORT, seed=BC.SEED + 1))


def test_refusals_launch_nothing_and_leave_the_context_usable():
    name = "fixed"
    eng, lp, n_roots, T = loaded(name)
    B = BC.bounds(name)
    starts = BC.starts(name, 2)
    good = eng.walk_bound(lp, starts, n_roots, T, B, BC.SEED, 256, SHORT)
    ms = eng.last_kernel_ms()
    assert ms > 0
    n_leaves, n_resid = len(lp.program.leaves), T.n_resid
    width = lp.program.leaves[0].width
    one = [(0, 0, 0, 1)]
    malformed = {
        "residual index": [(n_resid, [(0, 0, 0, 8)])],
        "no piece": [(0, [])],
        "65 pieces": [(0, one * 65)],
        "leaf index": [(0, [(n_leaves, 0, 0, 1)])],
        "leaf bits": [(0, [(0, width - 3, 0, 4)])],
        "value bits": [(0, [(0, 0, 253, 4)])],
        "len 0": [(0, [(0, 0, 0, 0)])],
        "257 entries": [(0, one)] * 257,
        "mode 5": [(0, one, 5, 0, 0)],
        "root truth at n_roots": [(0, one, RP.BOUND_LOW, n_roots, 0)],
        "atom truth at n_atoms": [(0, one, RP.BOUND_HIGH, RP.BOUND_ATOM | T.n_atoms, 0)],
        "an XOR entry with a truth": [(0, one, RP.BOUND_XOR, 1, 0)],
        "an XOR entry with fixed bits": [(0, one, RP.BOUND_XOR, 0, 1 << 200)],
    }
    bad = [dict(bounds=RP.make_bounds(m)) for m in malformed.values()]
    bad.append(dict(bounds=RP.Bounds(np.array([[0, 2, 2, 0, 0]], dtype=np.uint32), B.pieces[:3],
                                     np.zeros((1, 8), dtype=np.uint32), [0])))
    bad += [dict(starts=BC.starts(name, 65)), dict(n_roots=0), dict(lanes=0),
            dict(lanes=(1 << 20) + 1), dict(max_rounds=0), dict(n_resid=n_resid + 1)]
    for kw in bad:
        args = dict(starts=starts, n_roots=n_roots, trees=T, bounds=B, seed=BC.SEED, lanes=256,
                    max_rounds=SHORT)
        args.update(kw)
        with pytest.raises(EngineError, match=r"\(-1\): .*walk"):
            eng.walk_bound(lp, **args)
        assert eng.last_kernel_ms() == ms, kw             # no launch was timed
    # null tables with non-zero counts
    out = np.zeros_like(starts)
    nf, co = np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    nr, win = C.c_uint32(), C.c_uint32()
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    roots, atoms, code = (np.ascontiguousarray(a) for a in (T.roots, T.atoms, T.code))
    full = [eng._ctx, lp.handle, p(starts), 2, n_roots, 0, p(roots), T.n_atoms,
            p(atoms) if atoms.size else None, p(code) if code.size else None, len(code), n_resid,
            p(B.entries), len(B.entries), p(B.pieces), len(B.pieces), p(B.fixed), BC.SEED, 256,
            SHORT, 8, p(out), p(nf), p(co), C.byref(nr), None, C.byref(win)]
    for k in (12, 14, 16):
        q = list(full)
        q[k] = None
        assert eng.lib.mg_walk_bound(*q) == -1
        assert b"null" in eng.lib.mg_last_error(eng._ctx)
    assert eng.last_kernel_ms() == ms
    assert eng.lib.mg_walk_bound(*full) == 0
    assert nr.value == good.rounds and win.value == good.winner
    assert np.array_equal(out, good.leaves) and np.array_equal(nf, good.nfail)
    # and the next valid call succeeds
    same(eng.walk_bound(lp, starts, n_roots, T, B, BC.SEED, 256, SHORT), good)


def oracle_values(constraints, a):
    from oracle import smtlib_ref as R
    return R.evaluate(list(constraints), R.Assignment(a.vars, a.arrays, a.funcs))


# repair_group starts from the census's best candidate, a generated one: the
# side made of leaves is then about 128 bits from the other, as at the cases'
# own starts.  The aimed walk needs round 0 to learn the residuals and the
# masks, one aimed round per failing order (one, or two when the first lands
# past the window's other edge) and the plain moves of the guards; the plain
# moves gain about a bit per round on a MAGNITUDE distance of some 250.
GROUP_ROUNDS = {"window": 8, "signed": 8, "fixed": 8}


@pytest.mark.parametrize("name", BC.NAMES)
def test_repair_group_bound_solves_what_the_aim_cannot(name):
    cs, _ = BC.case(name)
    kw = dict(form="eval", max_rounds=GROUP_ROUNDS[name])
    assert kw["max_rounds"] <= 8
    g = RP.repair_group(cs, scored="bound", walkers=1, **kw)
    assert g["scoring"] == "bound" and len(g["bounds"]) == len(BC.bounds(name))
    assert g["bounds"].n_order == BC.bounds(name).n_order
    res = g["repair"]
    print(name, "starts", g.get("starts"), "rounds", res.rounds, "winner", res.winner,
          "trace", res.trace[res.winner, :res.rounds].tolist())
    aim = RP.repair_group(cs, scored="aim", walkers=1, **kw)         # the same rounds
    print(name, "aim:", aim["status"], "rounds", aim["repair"].rounds, "trace",
          aim["repair"].trace[0, :aim["repair"].rounds].tolist())
    assert g["status"] == RP.REPAIRED, (g["status"], g.get("why"))
    assert g["census"].n_sat == 0 and g["start"]["nfail"] > 0        # the generator missed
    assert res.nfail[res.winner] == 0 and res.rounds <= kw["max_rounds"]
    assert all(oracle_values(cs, g["assignment"]))
    assert aim["status"] == RP.STUCK and aim["scoring"] in ("aim", "tree")
    assert aim["repair"].nfail.min() > 0 and "assignment" not in aim and "bounds" not in aim


def window_query():
    """The `window` shape through the front-end with strict comparisons, so
    that no equality arm exists: h - 1 <u arg <u h + 4, arg the concat of 32
    byte symbols, with the guards of the crafted cases on h."""
    from mythril_amd.smt import Concat, Extract, Not, ULT, symbol_factory
    val = symbol_factory.BitVecVal
    h = symbol_factory.BitVecSym("bq_h", 256)
    arg = Concat(*[symbol_factory.BitVecSym("bq_b%02d" % i, 8) for i in reversed(range(32))])
    cons = [ULT(h - val(1, 256), arg), ULT(arg, h + val(4, 256))]
    cons += [Not(Extract(lo + 15, lo, h) == val(k, 16)) for lo in (64, 128) for k in (0, 0xFFFF)]
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


def test_get_model_repairs_a_window_query_with_the_bound_walk(model_state):
    M = model_state
    M.configure_from_env({"MYTHRIL_GPU_REPAIR": "5", "MYTHRIL_GPU_BUDGET_MS": "5000"})
    assert M.REPAIR and M.REPAIR_SCORED == "bound"
    cons = window_query()
    try:
        m = M.get_model(cons, enforce_execution_time=False)
    finally:
        M.SEARCH_BUDGET_MS = 200
    assert (M.stats.repair_attempts, M.stats.repair_hits) == (1, 1)
    assert M.stats.gpu_hits == 1 and not M._group_miss
    assert all(oracle_values([c.raw for c in cons], m.assignment))
    assert "GPU repair: attempts: 1 hits: 1" in M.stats.gpu_report()
    for value, want in (("4", "aim"), ("3", "tree"), ("2", True), ("1", False), ("0", False)):
        M.configure_from_env({"MYTHRIL_GPU_REPAIR": value})
        assert M.REPAIR_SCORED == want and M.REPAIR == (value != "0")


def test_get_model_misses_the_window_query_with_the_aimed_walk(model_state):
    """The same query, the same budget, MYTHRIL_GPU_REPAIR=4: no equality, so
    no aimed move, and the plain moves do not get there."""
    M = model_state
    M.configure_from_env({"MYTHRIL_GPU_REPAIR": "4", "MYTHRIL_GPU_BUDGET_MS": "5000"})
    assert M.REPAIR and M.REPAIR_SCORED == "aim"
    try:                                     # (z3 absent: nothing decides a miss)
        M.get_model(window_query(), enforce_execution_time=False)
    except M.SolverUnavailable:
        pass
    finally:
        M.SEARCH_BUDGET_MS = 200
    assert (M.stats.repair_attempts, M.stats.repair_hits) == (1, 0)
    assert M.stats.gpu_queries == 1 and M.stats.gpu_hits == 0 and M._group_miss

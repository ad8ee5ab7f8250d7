"""The walk with aims through sums on the GPU (mg_walk_sum,
csrc/mg_walk_sum.hip): Engine.walk_sum against walk_ref with
the tree scoring and the tables through the oracle (oracle/evalref.c) in every
output on the crafted cases (tests/sum_cases.py), on both register layouts, at
16 lanes (cap below the live list), 257 and 4096, at 1, 3 and 64 walkers and at
sync_every 1 and 8; on a generated case at the caps (64 side rows, 128 linear
entries); tables without a linear entry against Engine.walk_uf; the refusals
of the C ABI; repair_group(scored="sum") on the crafted cases, every model
checked by oracle/smtlib_ref.py; and MYTHRIL_GPU_REPAIR=7 through get_model on
a query of the `spend` shape in search form.  mg_walk_bound and mg_walk_uf run
the same kernels with narrower tables in the same workspace, so one test walks
down the rungs on one engine, each against its own reference."""

import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import bound_cases as BC
import sum_cases as SC
import tree_cases as TC
import uf_cases as UC
import walk_cases as WK
from mythril_amd import repair as RP
from mythril_amd.engine import EngineError, default_leafgen, get_engine

pytestmark = pytest.mark.gpu

SHORT = 8             # rounds at the shapes below the cases' own
# (lanes, walkers, sync_every) at SHORT rounds; 16 lanes: cap = 2 live lanes,
# below the live entries of `spend`
PLAN = ((16, 1, 8), (257, 3, 8), (256, 64, 8), (4096, 1, 1))


def loaded(name, nreg=16):
    """(engine of the layout, the case's walk view loaded with the default
    generator, root count, trees)."""
    prog = SC.program(name, nreg)
    ref = SC.program(name)                       # the reference ran on this program's tables
    assert prog.const_values == ref.const_values
    assert [(l.kind, l.source, l.chunk, l.entry, l.width) for l in prog.leaves] == \
        [(l.kind, l.source, l.chunk, l.entry, l.width) for l in ref.leaves]
    T = SC.trees(name)
    n_roots = len(SC.case(name)[0])
    view = SC.view(name, nreg)
    assert view.n_probes == SC.n_before(name) + SC.tables(name)[1].n_urows
    eng = get_engine(0, nreg=nreg)
    return eng, eng.load(view, default_leafgen(prog), prog_seed=0), n_roots, T


def same(got, want):
    assert np.array_equal(got.leaves, want.leaves)
    assert np.array_equal(got.nfail, want.nfail) and np.array_equal(got.cost, want.cost)
    assert got.winner == want.winner and got.rounds == want.rounds
    assert np.array_equal(got.trace, want.trace)


@pytest.mark.parametrize("nreg", (16, 11))
@pytest.mark.parametrize("name", SC.NAMES)
def test_walk_sum_equals_the_reference(name, nreg):
    eng, lp, n_roots, T = loaded(name, nreg)
    B, U, S = SC.tables(name)
    assert (S.n_linear > 0) == (name != "selector")
    for lanes, walkers, sync in PLAN:
        got = eng.walk_sum(lp, SC.starts(name, walkers), n_roots, T, B, U, S, SC.SEED, lanes,
                           SHORT, sync)
        same(got, SC.reference(name, walkers, lanes, SHORT, sync))
    # the case's own budget: the model the reference finds
    want = SC.reference(name)
    got = eng.walk_sum(lp, SC.starts(name, 1), n_roots, T, B, U, S, SC.SEED, SC.LANES,
                       SC.MAX_ROUNDS[name])
    same(got, want)
    assert got.nfail[0] == 0 and got.kernel_ms > 0


# ---------------------------------------------------------------------------
# generated: the caps
# ---------------------------------------------------------------------------

CAPS_SHAPES = ((64, 2), (300, 1))


@functools.lru_cache(maxsize=None)
def caps_reference(walkers, lanes):
    return SC.reference("caps", walkers, lanes, SC.MAX_ROUNDS["caps"])


def test_generated_case_at_the_caps_equals_the_reference():
    """64 linear XOR sides of two terms each: 64 side rows, 128 entries; the
    last side row and the per-walker row state at its largest."""
    eng, lp, n_roots, T = loaded("caps")
    B, U, S = SC.tables("caps")
    assert S.n_srows == RP.SUM_MAX_ROWS and len(B) == 128 == S.n_linear and n_roots == 64
    assert int(S.lin[-1]) >> RP.SUM_ROW_SHIFT == RP.SUM_MAX_ROWS - 1
    moved = 0
    for lanes, walkers in CAPS_SHAPES:
        got = eng.walk_sum(lp, SC.starts("caps", walkers), n_roots, T, B, U, S, SC.SEED, lanes,
                           SC.MAX_ROUNDS["caps"])
        want = caps_reference(walkers, lanes)
        same(got, want)
        moved += int(want.nfail[0] < n_roots - 1)
    assert moved                                         # aimed lanes were adopted


def test_a_table_without_a_linear_entry_is_walk_uf_bit_for_bit():
    """The tables of tests/uf_cases.py through the new entry point."""
    for name in UC.NAMES:
        prog = UC.program(name)
        T = UC.trees(name)
        B, U = UC.tables(name)
        eng = get_engine(0)
        lp = eng.load(UC.view(name), default_leafgen(prog), prog_seed=0)
        n_roots = len(UC.case(name)[0])
        none = RP.no_sums(len(B))
        for lanes, walkers in ((16, 2), (257, 3), (4096, 1)):
            starts = UC.starts(name, walkers)
            want = eng.walk_uf(lp, starts, n_roots, T, B, U, UC.SEED, lanes, SHORT)
            same(eng.walk_sum(lp, starts, n_roots, T, B, U, none, UC.SEED, lanes, SHORT), want)
    # and `selector`, whose table has plain entries from the new rules alone,
    # through the old entry point
    eng, lp, n_roots, T = loaded("selector")
    B, U, S = SC.tables("selector")
    starts = SC.starts("selector", 2)
    same(eng.walk_uf(lp, starts, n_roots, T, B, U, SC.SEED, 256, SHORT),
         eng.walk_sum(lp, starts, n_roots, T, B, U, S, SC.SEED, 256, SHORT))


def test_a_lower_rung_reads_nothing_a_higher_rung_left_in_the_workspace():
    """One engine, one workspace, down the rungs: linear entries and side rows,
    then slots and U rows without them, then neither, then no entry at all.
    3 walkers at 300 lanes: a full and a ragged tile each, several walker rows
    of every state array."""
    walkers, lanes = 3, 300
    eng = get_engine(0)
    load = lambda prog, view: eng.load(view, default_leafgen(prog), prog_seed=0)

    name = "sum"
    B, U, S = SC.tables(name)
    assert S.n_linear > 0 and S.n_srows > 0
    got = eng.walk_sum(load(SC.program(name), SC.view(name)), SC.starts(name, walkers),
                       len(SC.case(name)[0]), SC.trees(name), B, U, S, SC.SEED, lanes,
                       SC.MAX_ROUNDS[name])
    same(got, SC.reference(name, walkers, lanes, SC.MAX_ROUNDS[name]))

    name = "rekey"
    B, U = UC.tables(name)
    assert RP.has_slot_piece(B) and U.n_urows > 0
    got = eng.walk_uf(load(UC.program(name), UC.view(name)), UC.starts(name, walkers),
                      len(UC.case(name)[0]), UC.trees(name), B, U, UC.SEED, lanes,
                      UC.MAX_ROUNDS[name])
    same(got, UC.reference(name, walkers, lanes, UC.MAX_ROUNDS[name]))

    name = "signed"
    B = BC.bounds(name)
    assert B.n_order > 0
    lp = load(BC.program(name), BC.program(name))
    got = eng.walk_bound(lp, BC.starts(name, walkers), len(BC.case(name)[0]), BC.trees(name), B,
                         BC.SEED, lanes, BC.MAX_ROUNDS[name])
    same(got, BC.reference(name, walkers, lanes, BC.MAX_ROUNDS[name]))

    name = "nest"
    got = eng.walk_bound(load(TC.program(name), TC.program(name)), TC.starts(name, walkers),
                         len(TC.case(name)[0]), TC.trees(name), RP.make_bounds([]), TC.SEED, lanes, 16)
    same(got, TC.reference(name, walkers, lanes, 16))


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def test_refusals_launch_nothing_and_leave_the_context_usable():
    name = "sum"
    eng, lp, n_roots, T = loaded(name)
    B, U, S = SC.tables(name)
    starts = SC.starts(name, 2)
    good = eng.walk_sum(lp, starts, n_roots, T, B, U, S, SC.SEED, 256, SHORT)
    ms = eng.last_kernel_ms()
    assert ms > 0

    def lin(e, w, **kw):
        a = np.array(S.lin, dtype=np.uint32, copy=True)
        a[e] = w
        return dataclasses.replace(S, lin=a, **kw)
    slot_u = RP.make_ufs(slots=[(0, 0)], funcs=[(0, 1, 1)],
                         cands=[(0, RP.UF_ALWAYS, 0, 0, 0, 0)], n_urows=0)
    slot_b = RP.make_bounds([(0, [(RP.UF_SLOT | 0, 0, 0, 256)])], n_roots, T.n_atoms)
    bad = [dict(sums=lin(0, RP.SUM_NEG)),                            # a bad lin word
           dict(sums=lin(0, RP.SUM_LINEAR | 4)),
           dict(sums=lin(1, RP.SUM_LINEAR | 1 << 16)),
           dict(sums=lin(1, RP.SUM_LINEAR | S.n_srows << RP.SUM_ROW_SHIFT)),   # a side row at n_srows
           dict(sums=dataclasses.replace(S, n_srows=0)),
           dict(sums=dataclasses.replace(S, n_srows=RP.SUM_MAX_ROWS + 1)),
           dict(bounds=slot_b, ufs=slot_u, sums=RP.make_sums([(1, 0)], 1)),    # a slot piece
           dict(sums=dataclasses.replace(S, n_srows=S.n_srows + 1)),  # too few probes
           dict(ufs=dataclasses.replace(U, n_urows=1)),
           dict(starts=SC.starts(name, 65)), dict(n_roots=0), dict(lanes=0), dict(max_rounds=0)]
    for kw in bad:
        args = dict(starts=starts, n_roots=n_roots, trees=T, bounds=B, ufs=U, sums=S, seed=SC.SEED,
                    lanes=256, max_rounds=SHORT)
        args.update(kw)
        with pytest.raises(EngineError, match=r"\(-1\): .*walk"):
            eng.walk_sum(lp, **args)
        assert eng.last_kernel_ms() == ms, kw             # no launch was timed
    for kw in bad[:9]:                                    # the new checks say whose they are
        args = dict(starts=starts, n_roots=n_roots, trees=T, bounds=B, ufs=U, sums=S, seed=SC.SEED,
                    lanes=256, max_rounds=SHORT)
        args.update(kw)
        with pytest.raises(EngineError, match="walk_sum"):
            eng.walk_sum(lp, **args)
    # the slot piece is fine where the entry is not linear
    assert eng.last_kernel_ms() == ms
    # null tables with non-zero counts
    out = np.zeros_like(starts)
    nf, co = np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    nr, win = C.c_uint32(), C.c_uint32()
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    roots, atoms, code = (np.ascontiguousarray(a) for a in (T.roots, T.atoms, T.code))
    full = [eng._ctx, lp.handle, p(starts), 2, n_roots, 0, p(roots), T.n_atoms,
            p(atoms) if atoms.size else None, p(code) if code.size else None, len(code),
            T.n_resid, p(B.entries), len(B.entries), p(B.pieces), len(B.pieces), p(B.fixed),
            p(S.lin), S.n_srows, None, 0, None, 0, None, 0, None, 0, 0, SC.SEED, 256, SHORT, 8,
            p(out), p(nf), p(co), C.byref(nr), None, C.byref(win)]
    for k in (12, 14, 16, 17):
        q = list(full)
        q[k] = None
        assert eng.lib.mg_walk_sum(*q) == -1
        assert b"null" in eng.lib.mg_last_error(eng._ctx)
    q = list(full)
    q[20] = 1                                             # a slot count without slots
    assert eng.lib.mg_walk_sum(*q) == -1 and b"walk_sum" in eng.lib.mg_last_error(eng._ctx)
    assert eng.last_kernel_ms() == ms
    assert eng.lib.mg_walk_sum(*full) == 0
    assert nr.value == good.rounds and win.value == good.winner
    assert np.array_equal(out, good.leaves) and np.array_equal(nf, good.nfail)
    same(eng.walk_sum(lp, starts, n_roots, T, B, U, S, SC.SEED, 256, SHORT), good)


# ---------------------------------------------------------------------------
# repair_group and get_model
# ---------------------------------------------------------------------------

def oracle_values(constraints, a):
    from oracle import smtlib_ref as R
    return R.evaluate(list(constraints), R.Assignment(a.vars, a.arrays, a.funcs))


# repair_group starts from the census's best candidate, a generated one: round
# 0 learns the residuals, the masks and the side rows, then one aimed round per
# failing root that has an entry, and the plain moves for the guards a
# generated start breaks.
GROUP_ROUNDS = 8


@pytest.mark.parametrize("name", SC.STUCK)
def test_repair_group_sum_solves_what_the_uf_walk_cannot(name):
    cs, _ = SC.case(name)
    kw = dict(form="eval", max_rounds=GROUP_ROUNDS)
    g = RP.repair_group(cs, scored="sum", walkers=1, **kw)
    res = g["repair"]
    print(name, g["scoring"], "starts", g.get("starts"), "rounds", res.rounds, "trace",
          res.trace[res.winner, :res.rounds].tolist(), "linear", g["sums"].n_linear)
    old = RP.repair_group(cs, scored="uf", walkers=1, **kw)          # the same rounds
    print(name, "uf:", old["status"], old["scoring"], "trace",
          old["repair"].trace[0, :old["repair"].rounds].tolist())
    assert g["scoring"] == "sum" and g["sums"].n_linear >= 1
    assert len(g["sums"].lin) == len(g["bounds"])
    assert g["status"] == RP.REPAIRED, (g["status"], g.get("why"))
    assert g["census"].n_sat == 0 and g["start"]["nfail"] > 0        # the generator missed
    assert res.nfail[res.winner] == 0 and res.rounds <= GROUP_ROUNDS
    assert all(oracle_values(cs, g["assignment"]))
    assert old["status"] == RP.STUCK and old["scoring"] in ("uf", "bound", "aim", "tree")
    assert old["repair"].nfail.min() > 0 and "sums" not in old


SPENDS = 3


def spend_query():
    """The `spend` shape through the front-end, SPENDS times over one t: K <u
    s_i and s_i <=u t + 3, s_i = bal_i - v_i with the halves of bal_i
    exchanged, t = p xor q with p and q pinned to numerals and K = t - 1, so
    four values of each s_i make a model; bal_i and v_i carry the guards of
    tests/walk_cases.py.  Each order is some 250 bits from holding at a
    generated start and the plain moves gain about two bits a round, as
    tests/test_gpu_walk_uf.py measured for its `hash` query."""
    from mythril_amd.smt import Concat, Extract, Not, ULE, ULT, symbol_factory
    val = symbol_factory.BitVecVal
    sym = lambda s, w=256: symbol_factory.BitVecSym("sq_" + s, w)
    p, q = sym("p"), sym("q")
    rng = np.random.default_rng(0x7371)
    p0 = WK._guarded(int.from_bytes(rng.bytes(32), "little"), (64, 128))
    q0 = WK._guarded(int.from_bytes(rng.bytes(32), "little"), (64, 128)) ^ (
        0x1111 << 64 | 0x1111 << 128)
    K = (p0 ^ q0) - 1
    cons = [p == val(p0, 256), q == val(q0, 256)]
    for i in range(SPENDS):
        bal, v = sym("bal%d" % i), sym("v%d" % i)
        s = Concat(Extract(127, 0, bal), Extract(255, 128, bal)) - v
        cons += [ULT(val(K, 256), s), ULE(s, (p ^ q) + val(3, 256))]
        cons += [Not(Extract(lo + 15, lo, x) == val(k, 16)) for x in (bal, v) for lo in (64, 128)
                 for k in (0, 0xFFFF)]
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


def test_get_model_repairs_a_spend_query_with_the_sum_walk(model_state):
    M = model_state
    M.configure_from_env({"MYTHRIL_GPU_REPAIR": "7", "MYTHRIL_GPU_BUDGET_MS": "5000"})
    assert M.REPAIR and M.REPAIR_SCORED == "sum"
    cons = spend_query()
    try:
        m = M.get_model(cons, enforce_execution_time=False)
    finally:
        M.SEARCH_BUDGET_MS = 200
    assert (M.stats.repair_attempts, M.stats.repair_hits) == (1, 1)
    assert M.stats.gpu_hits == 1 and not M._group_miss
    assert all(oracle_values([c.raw for c in cons], m.assignment))
    for value, want in (("6", "uf"), ("5", "bound"), ("4", "aim"), ("3", "tree"), ("2", True),
                        ("1", False), ("0", False)):
        M.configure_from_env({"MYTHRIL_GPU_REPAIR": value})
        assert M.REPAIR_SCORED == want and M.REPAIR == (value != "0")


def test_get_model_misses_the_spend_query_with_the_uf_walk(model_state):
    """The same query, the same budget, MYTHRIL_GPU_REPAIR=6: no side of any
    order resolves without the linear rule, and the plain moves do not cover
    three differences' distances in 64 rounds."""
    M = model_state
    M.configure_from_env({"MYTHRIL_GPU_REPAIR": "6", "MYTHRIL_GPU_BUDGET_MS": "5000"})
    assert M.REPAIR and M.REPAIR_SCORED == "uf"
    try:                                     # (z3 absent: nothing decides a miss)
        M.get_model(spend_query(), enforce_execution_time=False)
    except M.SolverUnavailable:
        pass
    finally:
        M.SEARCH_BUDGET_MS = 200
    assert (M.stats.repair_attempts, M.stats.repair_hits) == (1, 0)
    assert M.stats.gpu_queries == 1 and M.stats.gpu_hits == 0 and M._group_miss

"""The tree-scored walk on the GPU (mg_walk_tree, csrc/mg_walk_tree.hip;
DESIGN.md §3.11): Engine.walk_tree against walk_ref with the tree scoring
through the oracle (oracle/evalref.c) in every output on the crafted cases
(tests/tree_cases.py), on both register layouts, at lane counts around the
wave and block sizes and at 1, 2, 3 and 64 walkers; the same walk with an INF
arm added to every program; an all-simple table against Engine.walk;
determinism; a start that is a model; the refusals of the C ABI;
repair_group(scored="tree") on the crafted cases, every model checked by
oracle/smtlib_ref.py; and MYTHRIL_GPU_REPAIR=3 through get_model."""

import ctypes as C
import types

import numpy as np
import pytest

import tree_cases as K
import walk_cases as WK
from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import EngineError, default_leafgen, get_engine

pytestmark = pytest.mark.gpu

SHORT = 8             # rounds at the shapes below the cases' own
# (lanes, walkers) at SHORT rounds; 64 walkers: at most 256 lanes
PLAN = ((1, 1), (1, 3), (63, 2), (64, 3), (65, 1), (256, 64), (1000, 2), (4096, 2))


def loaded(name, nreg=16):
    """(engine of the layout, the case's eval-form program with root mask,
    atom mask and residual probes loaded with the default generator, root
    count, trees)."""
    prog = K.program(name, nreg)
    ref = K.program(name)                        # the reference ran on this program's tables
    assert prog.const_values == ref.const_values and len(prog.leaves) == len(ref.leaves)
    T = K.trees(name)
    n_roots = len(K.case(name)[0])
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
@pytest.mark.parametrize("name", K.NAMES)
def test_walk_tree_equals_the_reference(name, nreg):
    eng, lp, n_roots, T = loaded(name, nreg)
    assert eng.nreg == nreg
    for lanes, walkers in PLAN:
        got = eng.walk_tree(lp, K.starts(name, walkers), n_roots, T, K.SEED, lanes, SHORT)
        want = K.reference(name, walkers, lanes, SHORT)
        assert got.trace.shape == (walkers, SHORT, 2) and got.leaves.shape == want.leaves.shape
        same(got, want)
        if lanes == 1:          # the start, with its own key, after every round
            assert np.array_equal(got.leaves, K.starts(name, walkers)) and got.rounds == SHORT
            assert (got.nfail == 1).all() and (got.cost > 50).all() and got.winner == 0
            assert (got.trace[:, :, 1] == got.cost[:, None]).all()
    got = eng.walk_tree(lp, K.starts(name, 1), n_roots, T, K.SEED, K.LANES, K.MAX_ROUNDS[name])
    same(got, K.reference(name))
    assert got.nfail[0] == 0 and got.rounds <= K.MAX_ROUNDS[name] // 2 and got.kernel_ms > 0


def with_inf_arms(T):
    """The same distances by longer programs: every tree root's value v
    becomes or(and(v), INF)."""
    roots, code = [], []
    for k, e in enumerate(T.roots):
        if not int(e) & RP.WT_TREE:
            roots.append(int(e))
            continue
        pc = int(e) & ~RP.WT_TREE
        roots.append(RP.WT_TREE | len(code))
        while int(T.code[pc]) >> 16 != RP.WT_END:
            code.append(int(T.code[pc]))
            pc += 1
        code += [RP.WT_AND << 16 | 1, RP.WT_PUSH_INF << 16, RP.WT_OR << 16 | 2, RP.WT_END << 16]
    return types.SimpleNamespace(roots=np.array(roots, dtype=np.uint32), atoms=T.atoms,
                                 code=np.array(code, dtype=np.uint32), probes=T.probes)


@pytest.mark.parametrize("name", K.NAMES)
def test_an_inf_arm_changes_nothing(name):
    eng, lp, n_roots, T = loaded(name)
    for lanes, walkers in ((65, 1), (1000, 2)):
        got = eng.walk_tree(lp, K.starts(name, walkers), n_roots, with_inf_arms(T), K.SEED, lanes,
                            SHORT)
        same(got, K.reference(name, walkers, lanes, SHORT))


@pytest.mark.parametrize("name", WK.NAMES)
def test_an_all_simple_table_is_the_table_walk(name):
    """No atoms, no code: mg_walk_tree on the programs of tests/walk_cases.py
    is mg_walk bit for bit."""
    prog = WK.program(name)
    probes, table = WK.scoring(name)
    n_roots = len(WK.case(name)[0])
    eng = get_engine(0, nreg=16)
    lp = eng.load(prog, default_leafgen(prog), prog_seed=0)
    T = RP.simple_trees(table)
    for lanes, walkers, rounds in ((1000, 3, SHORT), (WK.LANES, 1, WK.MAX_ROUNDS[name])):
        want = eng.walk(lp, WK.starts(name, walkers), n_roots, table, len(probes), WK.SEED, lanes,
                        rounds)
        got = eng.walk_tree(lp, WK.starts(name, walkers), n_roots, T, WK.SEED, lanes, rounds,
                            n_resid=len(probes))
        same(got, want)
    assert want.nfail[0] == 0


def test_two_runs_are_bit_identical():
    eng, lp, n_roots, T = loaded("nest")
    args = (lp, K.starts("nest", 3), n_roots, T)
    a = eng.walk_tree(*args, K.SEED, 1000, SHORT)
    b = eng.walk_tree(*args, K.SEED, 1000, SHORT)
    same(a, b)
    other = eng.walk_tree(*args, K.SEED + 1, 1000, SHORT)
    assert not np.array_equal(other.trace, a.trace) or not np.array_equal(other.leaves, a.leaves)


@pytest.mark.parametrize("name", K.NAMES)
def test_a_satisfying_start_returns_itself(name):
    eng, lp, n_roots, T = loaded(name)
    model = np.array(K.reference(name).leaves[0])
    starts = np.stack([K.start_rows(name), model])           # walker 1 starts at a model
    for sync in (1, 8):
        got = eng.walk_tree(lp, starts, n_roots, T, K.SEED, 256, K.MAX_ROUNDS[name], sync)
        assert np.array_equal(got.leaves[1], model) and got.nfail[1] == 0 == got.cost[1]
        assert got.rounds == sync and not got.trace[1].any() and got.winner == 1


def test_refusals_launch_nothing_and_leave_the_context_usable():
    name = "nest"
    eng, lp, n_roots, T = loaded(name)
    starts = K.starts(name, 2)
    good = eng.walk_tree(lp, starts, n_roots, T, K.SEED, 256, SHORT)
    ms = eng.last_kernel_ms()
    assert ms > 0

    def tables(**kw):
        d = dict(roots=np.array(T.roots), atoms=np.array(T.atoms), code=np.array(T.code),
                 probes=T.probes)
        d.update(kw)
        return types.SimpleNamespace(**d)

    def poke(a, i, v):
        a = np.array(a)
        a[i] = v
        return a
    n_code, n_atoms, n_resid = len(T.code), T.n_atoms, T.n_resid
    malformed = [
        tables(code=poke(T.code, 0, 7 << 16)),                              # unknown opcode
        tables(code=poke(T.code, 0, RP.WT_ATOM << 16 | n_atoms)),           # atom index
        tables(atoms=poke(T.atoms, 0, 3 << 16)),                            # atom kind
        tables(atoms=poke(T.atoms, 0, RP.HAMMING << 16 | n_resid)),         # residual index
        tables(roots=poke(T.roots, 1, RP.MAGNITUDE << 16 | n_resid)),       # a simple root's
        tables(roots=poke(T.roots, 0, RP.WT_TREE | n_code)),                # offset outside code
        tables(code=poke(T.code, n_code - 1, RP.WT_AND << 16 | 1)),         # no END
        tables(code=poke(T.code, 2, RP.WT_AND << 16 | 3)),                  # underflow
        tables(code=poke(T.code, n_code - 2, RP.WT_ATOM << 16)),            # two values at END
        tables(code=np.concatenate([np.full(9, RP.WT_PUSH_INF << 16, dtype=np.uint32),
                                    np.array([RP.WT_OR << 16 | 9, 0], dtype=np.uint32)])),
        tables(atoms=np.zeros(1025, dtype=np.uint32)),                      # 1025 atoms
        tables(atoms=np.zeros(257, dtype=np.uint32)),      # a second atom-mask probe: not there
    ]
    bad = [dict(starts=K.starts(name, 65)), dict(starts=starts[:0]), dict(n_roots=0),
           dict(n_roots=1025), dict(mask_probe0=1), dict(mask_probe0=9), dict(lanes=0),
           dict(lanes=(1 << 20) + 1), dict(max_rounds=0), dict(max_rounds=(1 << 16) + 1),
           dict(n_resid=n_resid + 1)] + [dict(trees=t) for t in malformed]
    for kw in bad:
        args = dict(starts=starts, n_roots=n_roots, trees=T, seed=K.SEED, lanes=256,
                    max_rounds=SHORT)
        args.update(kw)
        with pytest.raises(EngineError, match=r"\(-1\): .*walk"):
            eng.walk_tree(lp, **args)
        assert eng.last_kernel_ms() == ms, kw             # no launch was timed
    # null pointers (trace, and atoms / code of empty tables, may be null)
    out = np.zeros_like(starts)
    nf, co = np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    nr, win = C.c_uint32(), C.c_uint32()
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    roots, atoms, code = (np.ascontiguousarray(a) for a in (T.roots, T.atoms, T.code))
    full = [eng._ctx, lp.handle, p(starts), 2, n_roots, 0, p(roots), n_atoms, p(atoms), p(code),
            n_code, n_resid, K.SEED, 256, SHORT, 8, p(out), p(nf), p(co), C.byref(nr), None,
            C.byref(win)]
    for k in (1, 2, 6, 8, 9, 16, 17, 18, 19, 21):
        q = list(full)
        q[k] = None
        assert eng.lib.mg_walk_tree(*q) == -1 and b"null" in eng.lib.mg_last_error(eng._ctx)
    assert eng.last_kernel_ms() == ms
    assert eng.lib.mg_walk_tree(*full) == 0
    assert nr.value == good.rounds and win.value == good.winner
    assert np.array_equal(out, good.leaves) and np.array_equal(nf, good.nfail)
    assert np.array_equal(co, good.cost)
    # and the next valid call succeeds
    same(eng.walk_tree(lp, starts, n_roots, T, K.SEED, 256, SHORT), good)


def oracle_values(constraints, a):
    from oracle import smtlib_ref as R
    return R.evaluate(list(constraints), R.Assignment(a.vars, a.arrays, a.funcs))


# the census's best candidate is a generated one: every leaf of the equalities
# random, so about twice as far as the cases' own starts
GROUP_ROUNDS = {"chain": 256, "conj": 256, "nest": 384}


@pytest.mark.parametrize("name", K.NAMES)
def test_repair_group_tree_solves_what_the_table_cannot(name):
    cs, _ = K.case(name)
    kw = dict(form="eval", max_rounds=GROUP_ROUNDS[name])
    g = RP.repair_group(cs, scored="tree", walkers=4, **kw)
    assert g["scoring"] == "tree" and g["trees"].is_tree(0)
    res = g["repair"]
    print(name, "starts", g.get("starts"), "rounds", res.rounds, "winner", res.winner,
          "trace", res.trace[res.winner, :res.rounds:8].tolist())
    assert g["status"] == RP.REPAIRED, (g["status"], g.get("why"))
    assert g["census"].n_sat == 0 and g["start"]["nfail"] > 0        # the generator missed
    assert len(g["starts"]) == 4 == len(res.nfail) and g["starts"][0] == g["start"]["index"]
    assert res.nfail[res.winner] == 0 and res.rounds <= kw["max_rounds"]
    assert all(oracle_values(cs, g["assignment"]))
    table = RP.repair_group(cs, scored=True, walkers=4, **kw)        # today's table: stuck
    assert table["status"] == RP.STUCK and table["scoring"] == "count"
    assert table["repair"].nfail.min() > 0 and "assignment" not in table and "trees" not in table


def chain_query():
    """The `chain` shape through the front-end: m[arg] != 0 after one store
    m[h] = v into the zero array, arg the concat of 32 byte symbols, with the
    guards of the crafted cases on h."""
    from mythril_amd.smt import Concat, Extract, K as ConstArray, Not, symbol_factory
    val = symbol_factory.BitVecVal
    h, v = symbol_factory.BitVecSym("tq_h", 256), symbol_factory.BitVecSym("tq_v", 8)
    arg = Concat(*[symbol_factory.BitVecSym("tq_b%02d" % i, 8) for i in reversed(range(32))])
    m = ConstArray(256, 8, 0)
    m[h] = v
    cons = [Not(m[arg] == val(0, 8))]
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


def test_get_model_repairs_a_chain_query_with_the_tree_walk(model_state):
    M = model_state
    M.configure_from_env({"MYTHRIL_GPU_REPAIR": "3", "MYTHRIL_GPU_BUDGET_MS": "5000"})
    assert M.REPAIR and M.REPAIR_SCORED == "tree"
    cons = chain_query()
    try:
        m = M.get_model(cons, enforce_execution_time=False)
    finally:
        M.SEARCH_BUDGET_MS = 200
    assert (M.stats.repair_attempts, M.stats.repair_hits) == (1, 1)
    assert M.stats.gpu_hits == 1 and not M._group_miss
    assert all(oracle_values([c.raw for c in cons], m.assignment))
    assert "GPU repair: attempts: 1 hits: 1" in M.stats.gpu_report()
    for value, want in (("2", True), ("1", False), ("0", False)):
        M.configure_from_env({"MYTHRIL_GPU_REPAIR": value})
        assert M.REPAIR_SCORED is want and M.REPAIR == (value != "0")

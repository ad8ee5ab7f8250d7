"""The aimed walk on the GPU (mg_walk_aim, csrc/mg_walk_aim.hip; DESIGN.md
§3.12): Engine.walk_aim against walk_ref with the tree scoring and the aim
table through the oracle (oracle/evalref.c) in every output on the crafted
cases (tests/aim_cases.py), on both register layouts, at lane counts around
the wave and block sizes and at 1, 2, 3 and 64 walkers; an empty table against
Engine.walk_tree on the cases of tests/tree_cases.py; determinism; the
refusals of the C ABI; repair_group(scored="aim") on the crafted cases, every
model checked by oracle/smtlib_ref.py; and MYTHRIL_GPU_REPAIR=4 through
get_model."""

import ctypes as C

import numpy as np
import pytest

import aim_cases as AC
import tree_cases as K
from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import EngineError, default_leafgen, get_engine

pytestmark = pytest.mark.gpu

SHORT = 8             # rounds at the shapes below the cases' own
# (lanes, walkers) at SHORT rounds; 64 walkers: at most 256 lanes
PLAN = ((1, 1), (1, 3), (63, 2), (64, 3), (65, 1), (256, 64), (1000, 2), (4096, 2))


def loaded(name, nreg=16, cases=AC):
    """(engine of the layout, the case's eval-form program with root mask,
    atom mask and residual probes loaded with the default generator, root
    count, trees)."""
    prog = cases.program(name, nreg)
    ref = cases.program(name)                    # the reference ran on this program's tables
    assert prog.const_values == ref.const_values
    assert [(l.kind, l.source, l.chunk, l.width) for l in prog.leaves] == \
        [(l.kind, l.source, l.chunk, l.width) for l in ref.leaves]      # the aim table's leaves
    T = cases.trees(name)
    n_roots = len(cases.case(name)[0])
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
@pytest.mark.parametrize("name", AC.NAMES)
def test_walk_aim_equals_the_reference(name, nreg):
    eng, lp, n_roots, T = loaded(name, nreg)
    assert eng.nreg == nreg
    A = AC.aims(name)
    for lanes, walkers in PLAN:
        got = eng.walk_aim(lp, AC.starts(name, walkers), n_roots, T, A, AC.SEED, lanes, SHORT)
        want = AC.reference(name, walkers, lanes, SHORT)
        assert got.trace.shape == (walkers, SHORT, 2) and got.leaves.shape == want.leaves.shape
        same(got, want)
        if lanes == 1:          # the start, with its own key, after every round
            assert np.array_equal(got.leaves, AC.starts(name, walkers)) and got.rounds == SHORT
            assert (got.nfail == 1).all() and got.winner == 0
    got = eng.walk_aim(lp, AC.starts(name, 1), n_roots, T, A, AC.SEED, AC.LANES,
                       AC.MAX_ROUNDS[name])
    same(got, AC.reference(name))
    assert got.nfail[0] == 0 and got.rounds <= AC.MAX_ROUNDS[name] // 2 and got.kernel_ms > 0


@pytest.mark.parametrize("name", K.NAMES)
def test_an_empty_table_is_walk_tree_bit_for_bit(name):
    eng, lp, n_roots, T = loaded(name, 16, K)
    for lanes, walkers in ((64, 3), (1000, 2)):
        starts = K.starts(name, walkers)
        want = eng.walk_tree(lp, starts, n_roots, T, K.SEED, lanes, 16)
        same(eng.walk_aim(lp, starts, n_roots, T, RP.no_aims(), K.SEED, lanes, 16), want)
        same(want, K.reference(name, walkers, lanes, 16))


def test_two_runs_are_identical_and_another_seed_differs():
    name = "wide"
    eng, lp, n_roots, T = loaded(name)
    A = AC.aims(name)
    run = lambda seed: eng.walk_aim(lp, AC.starts(name, 3), n_roots, T, A, seed, 1000, 16)
    a, b, c = run(AC.SEED), run(AC.SEED), run(AC.SEED + 1)
    same(a, b)
    assert not np.array_equal(a.leaves, c.leaves)
    same(c, AC.reference(name, 3, 1000, 16, seed=AC.SEED + 1))


def test_refusals_launch_nothing_and_leave_the_context_usable():
    name = "odd"
    eng, lp, n_roots, T = loaded(name)
    A = AC.aims(name)
    starts = AC.starts(name, 2)
    good = eng.walk_aim(lp, starts, n_roots, T, A, AC.SEED, 256, SHORT)
    ms = eng.last_kernel_ms()
    assert ms > 0
    n_leaves, n_resid = len(lp.program.leaves), T.n_resid
    width = lp.program.leaves[0].width
    malformed = {
        "residual index": [(n_resid, [(0, 0, 0, 8)])],
        "no piece": [(0, [])],
        "65 pieces": [(0, [(0, 0, 0, 1)] * 65)],
        "leaf index": [(0, [(n_leaves, 0, 0, 1)])],
        "leaf bits": [(0, [(0, width - 3, 0, 4)])],
        "value bits": [(0, [(0, 0, 253, 4)])],
        "len 0": [(0, [(0, 0, 0, 0)])],
        "257 entries": [(0, [(0, 0, 0, 1)])] * 257,
    }
    bad = [dict(aims=RP.make_aims(m)) for m in malformed.values()]
    bad.append(dict(aims=RP.Aims(np.array([[0, 2, 2]], dtype=np.uint32), A.pieces, [0])))
    bad += [dict(starts=AC.starts(name, 65)), dict(n_roots=0), dict(lanes=0),
            dict(lanes=(1 << 20) + 1), dict(max_rounds=0), dict(n_resid=n_resid + 1)]
    for kw in bad:
        args = dict(starts=starts, n_roots=n_roots, trees=T, aims=A, seed=AC.SEED, lanes=256,
                    max_rounds=SHORT)
        args.update(kw)
        with pytest.raises(EngineError, match=r"\(-1\): .*walk"):
            eng.walk_aim(lp, **args)
        assert eng.last_kernel_ms() == ms, kw             # no launch was timed
    # null tables with non-zero counts
    out = np.zeros_like(starts)
    nf, co = np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    nr, win = C.c_uint32(), C.c_uint32()
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    roots, atoms, code = (np.ascontiguousarray(a) for a in (T.roots, T.atoms, T.code))
    full = [eng._ctx, lp.handle, p(starts), 2, n_roots, 0, p(roots), T.n_atoms,
            p(atoms) if atoms.size else None, p(code) if code.size else None, len(code), n_resid,
            p(A.entries), len(A.entries), p(A.pieces), len(A.pieces), AC.SEED, 256, SHORT, 8,
            p(out), p(nf), p(co), C.byref(nr), None, C.byref(win)]
    for k in (12, 14):
        q = list(full)
        q[k] = None
        assert eng.lib.mg_walk_aim(*q) == -1 and b"null" in eng.lib.mg_last_error(eng._ctx)
    assert eng.last_kernel_ms() == ms
    assert eng.lib.mg_walk_aim(*full) == 0
    assert nr.value == good.rounds and win.value == good.winner
    assert np.array_equal(out, good.leaves) and np.array_equal(nf, good.nfail)
    # and the next valid call succeeds
    same(eng.walk_aim(lp, starts, n_roots, T, A, AC.SEED, 256, SHORT), good)


def oracle_values(constraints, a):
    from oracle import smtlib_ref as R
    return R.evaluate(list(constraints), R.Assignment(a.vars, a.arrays, a.funcs))


# repair_group starts from the census's best candidate, a generated one, so the
# leaves of the equality are far from one another in every byte (a byte agrees
# with probability 1 / 256).  From such a start the coupling root fails too and
# does not trap the tree walk (measured once: from candidate 128 of `bytes` the
# tree walk repairs the group in 48 rounds of 4096 lanes), so what the tree
# walk cannot do is set by a count instead: a plain move corrects at most one
# of the differing bytes of a leaf — a LIMB move that sets four right has
# probability 2^-32 — unless a whole-leaf POOL or COPY finds the value
# somewhere, and a lane has two moves.  The budgets are half the rounds that
# count gives, or less:
#   bytes  32 one-byte leaves against h: 32 moves, 16 rounds; budget 8
#   odd    p (100 bits) against bits 156.. of x xor y xor z, which no leaf and
#          no pool value holds: 13 moves, 7 rounds; budget 4 (s may be one
#          COPY from z, q has 13 bits)
#   wide   two 256-bit chunks, 64 bytes: 32 rounds at two exact bytes per
#          round, 64 at one; budget 32.  (Copies between the generated leaves,
#          which share most of a word, do gain tens of bits in the first
#          rounds: measured 205, 134, 132, 78, then about one bit per round,
#          11 left after 32.)
# The aimed walk needs round 0 to learn the residuals, one aimed round per
# equality (wide: two chunks) and the plain moves of the rest of the case
# (bytes: v != 0; wide: h into its window).
GROUP_ROUNDS = {"bytes": 8, "wide": 32, "odd": 4}


@pytest.mark.parametrize("name", AC.NAMES)
def test_repair_group_aim_solves_what_the_tree_cannot(name):
    cs, _ = AC.case(name)
    kw = dict(form="eval", max_rounds=GROUP_ROUNDS[name])
    g = RP.repair_group(cs, scored="aim", walkers=1, **kw)
    assert g["scoring"] == "aim" and len(g["aims"]) == len(AC.aims(name))
    res = g["repair"]
    print(name, "starts", g.get("starts"), "rounds", res.rounds, "winner", res.winner,
          "trace", res.trace[res.winner, :res.rounds].tolist())
    tree = RP.repair_group(cs, scored="tree", walkers=1, **kw)       # the same rounds
    print(name, "tree:", tree["status"], "rounds", tree["repair"].rounds, "trace",
          tree["repair"].trace[0, :tree["repair"].rounds].tolist())
    assert g["status"] == RP.REPAIRED, (g["status"], g.get("why"))
    assert g["census"].n_sat == 0 and g["start"]["nfail"] > 0        # the generator missed
    assert res.nfail[res.winner] == 0 and res.rounds <= kw["max_rounds"]
    assert all(oracle_values(cs, g["assignment"]))
    assert tree["status"] == RP.STUCK and tree["scoring"] == "tree"
    assert tree["repair"].nfail.min() > 0 and "assignment" not in tree and "aims" not in tree


def bytes_query():
    """The `bytes` shape through the front-end: m[arg] != 0 after one store
    m[h] = v into the zero array, arg the concat of 32 byte symbols, the
    coupling root over bits 0..23 of arg xor h, with the guards of the crafted
    cases on h."""
    from mythril_amd.smt import Concat, Extract, K as ConstArray, Not, Or, symbol_factory
    val = symbol_factory.BitVecVal
    h, v = symbol_factory.BitVecSym("aq_h", 256), symbol_factory.BitVecSym("aq_v", 8)
    arg = Concat(*[symbol_factory.BitVecSym("aq_b%02d" % i, 8) for i in reversed(range(32))])
    m = ConstArray(256, 8, 0)
    m[h] = v
    blk = Extract(23, 0, arg ^ h)
    cons = [Not(m[arg] == val(0, 8)), Or(blk == val(0xFFFFFF, 24), blk == val(0, 24))]
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


def test_get_model_repairs_a_bytes_query_with_the_aimed_walk(model_state):
    M = model_state
    M.configure_from_env({"MYTHRIL_GPU_REPAIR": "4", "MYTHRIL_GPU_BUDGET_MS": "5000"})
    assert M.REPAIR and M.REPAIR_SCORED == "aim"
    cons = bytes_query()
    try:
        m = M.get_model(cons, enforce_execution_time=False)
    finally:
        M.SEARCH_BUDGET_MS = 200
    assert (M.stats.repair_attempts, M.stats.repair_hits) == (1, 1)
    assert M.stats.gpu_hits == 1 and not M._group_miss
    assert all(oracle_values([c.raw for c in cons], m.assignment))
    assert "GPU repair: attempts: 1 hits: 1" in M.stats.gpu_report()
    for value, want in (("3", "tree"), ("2", True), ("1", False), ("0", False)):
        M.configure_from_env({"MYTHRIL_GPU_REPAIR": value})
        assert M.REPAIR_SCORED == want and M.REPAIR == (value != "0")

"""The walk with aims for UF outputs on the GPU (mg_walk_uf,
csrc/mg_walk_uf.hip): Engine.walk_uf against walk_ref with
the tree scoring and the tables through the oracle (oracle/evalref.c) in every
output on the crafted cases (tests/uf_cases.py), on both register layouts, at
16 lanes (cap below the live list), 257 and 4096, at 1, 3 and 64 walkers and at
sync_every 1 and 8; on generated cases with 64 slots (two-chunk keys, 128 U
rows) and with three-chunk keys; a slot-free table against Engine.walk_bound;
the refusals of the C ABI; repair_group(scored="uf") on the crafted cases,
every model checked by oracle/smtlib_ref.py; and MYTHRIL_GPU_REPAIR=6 through
get_model on a query of the `hash` shape (search form: PROBE keys)."""

import ctypes as C
import functools

import numpy as np
import pytest

import aim_cases as AC
import tree_cases as TC
import uf_cases as UC
import walk_cases as WK
from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import EngineError, default_leafgen, get_engine
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N
from oracle import evalref

pytestmark = pytest.mark.gpu

SHORT = 8             # rounds at the shapes below the cases' own
# (lanes, walkers, sync_every) at SHORT rounds; 16 lanes: cap = 2 live lanes,
# below the live entries of `rekey` and `hash`
PLAN = ((16, 1, 8), (257, 3, 8), (256, 64, 8), (4096, 1, 1))


def loaded(name, nreg=16):
    """(engine of the layout, the case's walk view loaded with the default
    generator, root count, trees)."""
    prog = UC.program(name, nreg)
    ref = UC.program(name)                       # the reference ran on this program's tables
    assert prog.const_values == ref.const_values
    assert [(l.kind, l.source, l.chunk, l.entry, l.width) for l in prog.leaves] == \
        [(l.kind, l.source, l.chunk, l.entry, l.width) for l in ref.leaves]
    T = UC.trees(name)
    n_roots = len(UC.case(name)[0])
    view = UC.view(name, nreg)
    assert view.n_probes == UC.n_before(name) + UC.tables(name)[1].n_urows
    eng = get_engine(0, nreg=nreg)
    return eng, eng.load(view, default_leafgen(prog), prog_seed=0), n_roots, T


def same(got, want):
    assert np.array_equal(got.leaves, want.leaves)
    assert np.array_equal(got.nfail, want.nfail) and np.array_equal(got.cost, want.cost)
    assert got.winner == want.winner and got.rounds == want.rounds
    assert np.array_equal(got.trace, want.trace)


@pytest.mark.parametrize("nreg", (16, 11))
@pytest.mark.parametrize("name", UC.NAMES)
def test_walk_uf_equals_the_reference(name, nreg):
    eng, lp, n_roots, T = loaded(name, nreg)
    B, U = UC.tables(name)
    assert RP.has_slot_piece(B)
    for lanes, walkers, sync in PLAN:
        got = eng.walk_uf(lp, UC.starts(name, walkers), n_roots, T, B, U, UC.SEED, lanes, SHORT,
                          sync)
        same(got, UC.reference(name, walkers, lanes, SHORT, sync))
    # the case's own budget: the model the reference finds
    want = UC.reference(name)
    got = eng.walk_uf(lp, UC.starts(name, 1), n_roots, T, B, U, UC.SEED, UC.LANES,
                      UC.MAX_ROUNDS[name])
    same(got, want)
    assert got.nfail[0] == 0 and got.kernel_ms > 0


# ---------------------------------------------------------------------------
# generated: many slots, wide keys
# ---------------------------------------------------------------------------

GEN = {"s64c2": (64, 2), "s40c3": (40, 3)}            # slots, key chunks
GEN_SEED, GEN_ROUNDS = 0x7566, 4
GEN_SHAPES = ((64, 2), (300, 1))


@functools.lru_cache(maxsize=None)
def gen_built(name):
    """n roots f(concat(x_i, y)) = p_i: n slots of one function, every key
    `chunks` chunks wide, n + .. leaves."""
    n, chunks = GEN[name]
    with N.fresh_scope():
        y = N.bv_var("y", 256 * (chunks - 1) + 100)
        apps = [N.apply_uf("f", y.width + 8, 256, N.concat(N.bv_var("x%02d" % i, 8), y))
                for i in range(n)]
        cs = [N.eq(a, N.bv_var("p%02d" % i, 256)) for i, a in enumerate(apps)]
        T = RP.distance_trees(cs)
        mask, amask = CS.mask_probes(cs), CS.mask_probes(T.atom_nodes)
        kept, up = RP.uf_probes(T)
    prog = compile_constraints(cs, mask + amask + list(T.probes) + list(up))
    B, U = RP.uf_table(cs, T, prog, kept)
    S = evalref.serialize(cs, prog, list(T.atom_nodes) + list(T.probes) + list(up))
    records = [S.node_index[v.id] for v in list(cs) + list(T.atom_nodes) + list(T.probes)
               + list(up)]
    n_c, n_a, n_r = len(cs), len(T.atom_nodes), len(T.probes)

    def values_fn(soa):
        _, vals = evalref.run_nodes_soa(S, prog, np.ascontiguousarray(soa), records=records,
                                        chunk=256)
        return ((vals[:, :n_c, 0] & np.uint64(1)).astype(bool),
                (vals[:, n_c:n_c + n_a, 0] & np.uint64(1)).astype(bool),
                TC._rows(vals[:, n_c + n_a:n_c + n_a + n_r]), TC._rows(vals[:, n_c + n_a + n_r:]))
    rng = np.random.default_rng(GEN_SEED)
    start = np.zeros((len(prog.leaves), 8), dtype=np.uint32)
    for i, leaf in enumerate(prog.leaves):
        v = int.from_bytes(rng.bytes(32), "little") & ((1 << leaf.width) - 1)
        start[i] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    view = RP.uf_view(prog, n_c_probes(cs, T) + U.n_arg_rows, U.keep)
    return cs, prog, T, B, U, values_fn, start, view


def n_c_probes(cs, T):
    return CS.n_mask_probes(len(cs)) + CS.n_mask_probes(T.n_atoms) + T.n_resid


@functools.lru_cache(maxsize=None)
def gen_reference(name, walkers, lanes):
    cs, prog, T, B, U, values_fn, start, _ = gen_built(name)
    return RP.walk_ref(values_fn, default_leafgen(prog), WK.consts_of(prog),
                       np.repeat(start[None], walkers, axis=0), T.roots, GEN_SEED, lanes,
                       GEN_ROUNDS, 8, score=RP.tree_scoring(T), bounds=B, ufs=U)


@pytest.mark.parametrize("name", sorted(GEN))
def test_generated_cases_equal_the_reference(name):
    cs, prog, T, B, U, _, start, view = gen_built(name)
    n, chunks = GEN[name]
    assert len(U) == n and U.n_urows == n * chunks and int(U.funcs[0, 2]) == chunks
    if name == "s64c2":                                  # both caps, the last slot thread
        assert len(U) == RP.UF_MAX_SLOTS and U.n_urows == RP.UF_MAX_ROWS
    slot_pieces = B.pieces[(B.pieces[:, 0] & RP.UF_SLOT) != 0, 0] & ~np.uint32(RP.UF_SLOT)
    assert sorted(set(slot_pieces.tolist())) == list(range(n))
    eng = get_engine(0)
    lp = eng.load(view, default_leafgen(prog), prog_seed=0)
    moved = 0
    for lanes, walkers in GEN_SHAPES:
        got = eng.walk_uf(lp, np.repeat(start[None], walkers, axis=0), len(cs), T, B, U, GEN_SEED,
                          lanes, GEN_ROUNDS)
        want = gen_reference(name, walkers, lanes)
        same(got, want)
        moved += int(want.nfail[0] < len(cs))
    assert moved                                         # aimed lanes were adopted


def test_a_slot_free_table_is_walk_bound_bit_for_bit():
    import bound_cases as BC
    for name in ("signed", "fixed"):
        prog = BC.program(name)
        T, B = BC.trees(name), BC.bounds(name)
        eng = get_engine(0)
        lp = eng.load(prog, default_leafgen(prog), prog_seed=0)
        n_roots = len(BC.case(name)[0])
        for lanes, walkers in ((16, 2), (257, 3), (4096, 1)):
            starts = BC.starts(name, walkers)
            want = eng.walk_bound(lp, starts, n_roots, T, B, BC.SEED, lanes, SHORT)
            same(eng.walk_uf(lp, starts, n_roots, T, B, RP.no_ufs(), BC.SEED, lanes, SHORT), want)
    name = "bytes"                                       # XOR entries only
    prog, T, A = AC.program(name), AC.trees(name), AC.aims(name)
    B = RP.bounds_of_aims(A, len(T.roots), T.n_atoms)
    eng = get_engine(0)
    lp = eng.load(prog, default_leafgen(prog), prog_seed=0)
    starts = AC.starts(name, 2)
    same(eng.walk_uf(lp, starts, len(T.roots), T, B, RP.no_ufs(), AC.SEED, 256, SHORT),
         eng.walk_bound(lp, starts, len(T.roots), T, B, AC.SEED, 256, SHORT))


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def test_refusals_launch_nothing_and_leave_the_context_usable():
    import dataclasses
    name = "shadow"
    eng, lp, n_roots, T = loaded(name)
    B, U = UC.tables(name)
    starts = UC.starts(name, 2)
    good = eng.walk_uf(lp, starts, n_roots, T, B, U, UC.SEED, 256, SHORT)
    ms = eng.last_kernel_ms()
    assert ms > 0
    n_leaves = len(lp.program.leaves)

    def changed(table, row, col, value):
        a = np.array(getattr(U, table), dtype=np.uint32, copy=True)
        a[row, col] = value
        return dataclasses.replace(U, **{table: a})
    narrow = next(i for i, l in enumerate(lp.program.leaves) if l.width < 256) \
        if any(l.width < 256 for l in lp.program.leaves) else None
    bad = [dict(ufs=changed("slots", 0, 0, len(U.funcs))),           # function index
           dict(ufs=changed("slots", 1, 1, U.n_urows)),              # argument row
           dict(ufs=changed("funcs", 0, 2, 0)), dict(ufs=changed("funcs", 0, 2, 5)),
           dict(ufs=changed("funcs", 0, 1, len(U.cands) + 1)),       # candidates past the table
           dict(ufs=changed("cands", 0, 0, n_leaves)),               # value leaf
           dict(ufs=changed("cands", 0, 1, 4)),                      # key kind
           dict(ufs=changed("cands", 0, 2, n_leaves)),               # LEAF key
           dict(ufs=changed("cands", 0, slice(1, 3), (RP.UF_PROBE, U.n_urows))),    # PROBE key
           dict(ufs=changed("cands", 0, 1, RP.UF_CONST)),            # CONST key, no ukeys
           dict(ufs=dataclasses.replace(U, n_urows=U.n_urows + 1)),  # rows the program lacks
           dict(ufs=dataclasses.replace(U, n_urows=RP.UF_MAX_ROWS + 1)),
           dict(bounds=RP.make_bounds([(0, [(RP.UF_SLOT | len(U), 0, 0, 8)])])),    # slot index
           dict(bounds=RP.make_bounds([(0, [(RP.UF_SLOT | 0, 250, 0, 8)])])),       # past the width
           dict(starts=UC.starts(name, 65)), dict(n_roots=0), dict(lanes=0), dict(max_rounds=0)]
    if narrow is not None:                                           # value leaves of two widths
        bad.append(dict(ufs=changed("cands", 1, 0, narrow)))
    for kw in bad:
        args = dict(starts=starts, n_roots=n_roots, trees=T, bounds=B, ufs=U, seed=UC.SEED,
                    lanes=256, max_rounds=SHORT)
        args.update(kw)
        with pytest.raises(EngineError, match=r"\(-1\): .*walk"):
            eng.walk_uf(lp, **args)
        assert eng.last_kernel_ms() == ms, kw             # no launch was timed
    # null tables with non-zero counts
    out = np.zeros_like(starts)
    nf, co = np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    nr, win = C.c_uint32(), C.c_uint32()
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    roots, atoms, code = (np.ascontiguousarray(a) for a in (T.roots, T.atoms, T.code))
    full = [eng._ctx, lp.handle, p(starts), 2, n_roots, 0, p(roots), T.n_atoms,
            p(atoms) if atoms.size else None, p(code) if code.size else None, len(code),
            T.n_resid, p(B.entries), len(B.entries), p(B.pieces), len(B.pieces), p(B.fixed),
            p(U.slots), len(U.slots), p(U.funcs), len(U.funcs), p(U.cands), len(U.cands), None, 0,
            U.n_urows, UC.SEED, 256, SHORT, 8, p(out), p(nf), p(co), C.byref(nr), None,
            C.byref(win)]
    for k in (12, 14, 16, 17, 19, 21):
        q = list(full)
        q[k] = None
        assert eng.lib.mg_walk_uf(*q) == -1
        assert b"null" in eng.lib.mg_last_error(eng._ctx)
    assert eng.last_kernel_ms() == ms
    assert eng.lib.mg_walk_uf(*full) == 0
    assert nr.value == good.rounds and win.value == good.winner
    assert np.array_equal(out, good.leaves) and np.array_equal(nf, good.nfail)
    same(eng.walk_uf(lp, starts, n_roots, T, B, U, UC.SEED, 256, SHORT), good)


# ---------------------------------------------------------------------------
# repair_group and get_model
# ---------------------------------------------------------------------------

def oracle_values(constraints, a):
    from oracle import smtlib_ref as R
    return R.evaluate(list(constraints), R.Assignment(a.vars, a.arrays, a.funcs))


# repair_group starts from the census's best candidate, a generated one: round
# 0 learns the residuals, the masks and the destinations, then one aimed round
# per failing root that has an entry (at most 4 in `hash`, 3 in `rekey`), and
# the plain moves for the guards a generated start breaks.
GROUP_ROUNDS = 8
# `ckey` is a case only as compiled with constant keys, which repair_group's
# eval form never asks for (there f(7) is a lookup at a numeral argument, which
# gets no slot) and whose search form defines f(7) := p xor q by construction,
# so that no walk starts; the walks of `ckey` are compared above.
GROUP_NAMES = tuple(n for n in UC.NAMES if n != "ckey")


@pytest.mark.parametrize("name", GROUP_NAMES)
def test_repair_group_uf_solves_what_the_bound_walk_cannot(name):
    cs, _ = UC.case(name)
    kw = dict(form="eval", max_rounds=GROUP_ROUNDS)
    g = RP.repair_group(cs, scored="uf", walkers=1, **kw)
    res = g["repair"]
    print(name, g["scoring"], "starts", g.get("starts"), "rounds", res.rounds, "trace",
          res.trace[res.winner, :res.rounds].tolist(), "slots", len(g["ufs"]))
    bound = RP.repair_group(cs, scored="bound", walkers=1, **kw)     # the same rounds
    print(name, "bound:", bound["status"], bound["scoring"], "trace",
          bound["repair"].trace[0, :bound["repair"].rounds].tolist())
    assert g["scoring"] == "uf" and len(g["ufs"]) >= 1 and RP.has_slot_piece(g["bounds"])
    assert g["status"] == RP.REPAIRED, (g["status"], g.get("why"))
    assert g["census"].n_sat == 0 and g["start"]["nfail"] > 0        # the generator missed
    assert res.nfail[res.winner] == 0 and res.rounds <= GROUP_ROUNDS
    assert all(oracle_values(cs, g["assignment"]))
    assert bound["status"] == RP.STUCK and bound["scoring"] in ("bound", "aim", "tree")
    assert bound["repair"].nfail.min() > 0 and "ufs" not in bound


HASHES = 3


def hash_query():
    """The `hash` shape through the front-end, HASHES times over one t: K <u
    h_i and h_i <=u t + 3, h_i = f_i(concat(x_i, y)) with its halves exchanged,
    t = p xor q with p and q pinned to numerals and K = t - 1, so four values
    of each h_i make a model.  (One such pair is within the slot-free walk's
    reach: from the census's start, a pool value of the entry, it is some 112
    bits away and the plain moves gain about two bits a round, 53 of the 64
    rounds; so are three applications of one function, which the start keys
    alike and so reads from one entry: 1 bit short after 64 rounds.  Three
    functions are three entries, three times as far: measured, the slot-free
    walk goes from (3, 345) to (3, 70) in 64 rounds of 16 walkers, the UF walk
    to (0, 0) in round 3.)"""
    from mythril_amd.smt import Concat, Extract, Function, Not, ULE, ULT, symbol_factory
    val = symbol_factory.BitVecVal
    sym = lambda s, w=256: symbol_factory.BitVecSym("uq_" + s, w)
    y, p, q = sym("y"), sym("p"), sym("q")
    rng = np.random.default_rng(0x6871)
    p0 = WK._guarded(int.from_bytes(rng.bytes(32), "little"), (64, 128))
    q0 = WK._guarded(int.from_bytes(rng.bytes(32), "little"), (64, 128)) ^ (
        0x1111 << 64 | 0x1111 << 128)
    K = (p0 ^ q0) - 1
    cons = [p == val(p0, 256), q == val(q0, 256)]
    cons += [Not(Extract(lo + 15, lo, v) == val(k, 16)) for v in (p, q) for lo in (64, 128)
             for k in (0, 0xFFFF)]
    for i in range(HASHES):
        fw = Function("uq_f%d" % i, 512, 256)(Concat(sym("x%d" % i), y))
        h = Concat(Extract(127, 0, fw), Extract(255, 128, fw))
        cons += [ULT(val(K, 256), h), ULE(h, (p ^ q) + val(3, 256))]
        cons += [Not(Extract(lo + 15, lo, h) == val(k, 16)) for lo in (64, 128)
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


def test_get_model_repairs_a_hash_query_with_the_uf_walk(model_state):
    M = model_state
    M.configure_from_env({"MYTHRIL_GPU_REPAIR": "6", "MYTHRIL_GPU_BUDGET_MS": "5000"})
    assert M.REPAIR and M.REPAIR_SCORED == "uf"
    cons = hash_query()
    try:
        m = M.get_model(cons, enforce_execution_time=False)
    finally:
        M.SEARCH_BUDGET_MS = 200
    assert (M.stats.repair_attempts, M.stats.repair_hits) == (1, 1)
    assert M.stats.gpu_hits == 1 and not M._group_miss
    assert all(oracle_values([c.raw for c in cons], m.assignment))
    for value, want in (("5", "bound"), ("4", "aim"), ("3", "tree"), ("2", True), ("1", False),
                        ("0", False)):
        M.configure_from_env({"MYTHRIL_GPU_REPAIR": value})
        assert M.REPAIR_SCORED == want and M.REPAIR == (value != "0")


def test_get_model_misses_the_hash_query_with_the_bound_walk(model_state):
    """The same query, the same budget, MYTHRIL_GPU_REPAIR=5: no side of
    any order resolves without a slot, and the plain moves do not cover three
    entries' distances in 64 rounds."""
    M = model_state
    M.configure_from_env({"MYTHRIL_GPU_REPAIR": "5", "MYTHRIL_GPU_BUDGET_MS": "5000"})
    assert M.REPAIR and M.REPAIR_SCORED == "bound"
    try:                                     # (z3 absent: nothing decides a miss)
        M.get_model(hash_query(), enforce_execution_time=False)
    except M.SolverUnavailable:
        pass
    finally:
        M.SEARCH_BUDGET_MS = 200
    assert (M.stats.repair_attempts, M.stats.repair_hits) == (1, 0)
    assert M.stats.gpu_queries == 1 and M.stats.gpu_hits == 0 and M._group_miss

"""CPU tests of the walk with aims for UF outputs: the
conditions on the crafted cases of tests/uf_cases.py, the applications and
argument probes of ``repair.uf_probes``, the tables of ``repair.uf_table`` in
eval and solve form, the walk view, the library's resolver and lane function
(csrc/mg_walk_uf.h through mg_walk_uf_resolve_host and mg_walk_uf_mutate_host)
against ``repair.uf_resolve_ref`` and ``repair.uf_mutate_ref`` limb for limb on
the cases and on synthetic tables of every key kind, the slot-free walk against
the walk of §3.13, the assumption the solve-form tables rest on (an argument
probe equals its own entry's key probe), and the validator's refusals.  No
GPU."""

import dataclasses

import numpy as np
import pytest

import bound_cases as BC
import ir_sim
import uf_cases as UC
from mythril_amd import census as CS
from mythril_amd import irdefs as I
from mythril_amd import repair as RP
from mythril_amd.engine import (EngineError, LeafGen, default_leafgen, walk_bound_mutate_host,
                                walk_uf_mutate_host, walk_uf_resolve_host)
from mythril_amd.ir import compile_constraints
from mythril_amd.model import _compile_search_uncached
from mythril_amd.smt import node as N

NONE = RP.AIM_NONE
SLOT = RP.UF_SLOT


# ---------------------------------------------------------------------------
# the crafted cases
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", UC.NAMES)
def test_crafted_cases_need_the_uf_aims(name):
    """The conditions on the inputs, none of them a measurement: (a) the
    generator finds no model among lanes x max_rounds candidates, (b) walk_ref
    with the tree scoring and the table of §3.13 is still failing after
    max_rounds from the same start, (c) with the tables of §3.14 it reaches a
    model within half of max_rounds."""
    rounds = UC.MAX_ROUNDS[name]
    B, U = UC.tables(name)
    prog = UC.program(name)
    leaf = {l.name: i for i, l in enumerate(prog.leaves)}
    start = UC.start_rows(name)
    values = UC.values_fn(name)(start[:, :, None])
    dest = RP.uf_resolve_ref(start, values[3][:, :, 0], U).tolist()
    kinds = [int(k) for k in U.cands[:, 1]]
    if name == "hash":
        assert len(U) == 1 and U.n_urows == 2 and int(U.funcs[0, 2]) == 2     # a 512-bit key
        assert kinds == [RP.UF_LEAF, RP.UF_LEAF, RP.UF_ALWAYS]
        assert dest == [leaf["f#else#0"]]                # no key leaf equals w
        # p and q (leaf pieces), then both orders by their UF side alone: the
        # two halves of the slot, exchanged
        assert [int(m) for m in B.entries[:, 3]] == [RP.BOUND_XOR, RP.BOUND_XOR,
                                                     RP.BOUND_HIGH_STRICT, RP.BOUND_LOW]
        assert B.of(2) == B.of(3) == [(SLOT | 0, 0, 128, 128), (SLOT | 0, 128, 0, 128)]
        assert len(UC.bounds(name)) == 2 and UC.bounds(name).n_order == 0
    elif name in ("shadow", "rekey"):
        assert len(U) == 2 and kinds == [RP.UF_LEAF, RP.UF_LEAF, RP.UF_ALWAYS]
        assert [B.of(e) for e in (0, 1)] == [[(SLOT | 0, 0, 0, 256)], [(SLOT | 1, 0, 0, 256)]]
        # first match: entries 0 and 1 both equal a; b reads else.  rekey: nothing matches
        assert dest == ([leaf["f#v0#0"], leaf["f#else#0"]] if name == "shadow"
                        else [leaf["f#else#0"]] * 2)
        assert len(UC.bounds(name)) == (0 if name == "shadow" else 2)
    else:
        assert prog.table_ckeys == {"f": [7]} and len(U) == 1 and len(U.ukeys) == 1
        assert kinds == [RP.UF_CONST, RP.UF_LEAF, RP.UF_LEAF, RP.UF_ALWAYS]
        assert B.of(0) == [(leaf["f#c0#0"], 0, 0, 256)]  # f(7): statically the cval leaf
        assert B.of(1) == [(SLOT | 0, 0, 0, 256)] and dest == [leaf["f#else#0"]]
        assert len(UC.bounds(name)) == 0                 # §3.13 resolves no application
    assert (~values[0][0]).sum() in (1, 2)
    assert UC.generator_hits(name, UC.LANES * rounds) == 0                        # (a)
    stuck = UC.reference(name, uf=False)
    assert stuck.nfail[0] > 0 and stuck.rounds == rounds                          # (b)
    res = UC.reference(name)
    zero = np.flatnonzero(res.trace[0, :res.rounds, 0] == 0)
    assert zero.size and int(zero[0]) < rounds // 2                               # (c)
    assert int(zero[0]) == UC.FIRST_ZERO[name]           # what the cases' docstring says
    assert res.nfail[0] == 0 == res.cost[0] and res.winner == 0 and res.rounds % 8 == 0
    assert UC.values_fn(name)(np.asarray(res.leaves[0])[:, :, None])[0].all()


def test_rekey_resolves_again_after_the_first_adoption():
    """Round 0 adopts the copy of d to c, round 1 the plain move that makes
    entry 0's key equal a; round 2's aimed move must then write v0, the
    destination resolved at round 1's adoption."""
    res = UC.reference("rekey")
    assert res.trace[0, :3].tolist()[2] == [0, 0] and res.trace[0, 0, 0] == res.trace[0, 1, 0] == 1
    prog = UC.program("rekey")
    leaf = {l.name: i for i, l in enumerate(prog.leaves)}
    start, end = UC.start_rows("rekey"), np.asarray(res.leaves[0])
    changed = {l.name for i, l in enumerate(prog.leaves) if (start[i] != end[i]).any()}
    assert "f#v0#0" in changed and "f#else#0" not in changed
    assert (end[leaf["f#k0#0"]] == end[leaf["a"]]).all() and \
        (start[leaf["f#k0#0"]] != start[leaf["a"]]).any()


def test_with_no_slot_walk_ref_is_the_walk_of_bounds():
    name = "signed"
    prog, T, B = BC.program(name), BC.trees(name), BC.bounds(name)
    want = BC.reference(name, 2, 256, 8)
    fn = BC.values_fn(name)
    with_rows = lambda soa: fn(soa) + (np.zeros((0, 8, soa.shape[2]), dtype=np.uint32),)
    got = RP.walk_ref(with_rows, default_leafgen(prog), BC.consts_of(prog), BC.starts(name, 2),
                      T.roots, BC.SEED, 256, 8, 8, score=RP.tree_scoring(T), bounds=B,
                      ufs=RP.no_ufs())
    for a, b in ((got.leaves, want.leaves), (got.nfail, want.nfail), (got.cost, want.cost),
                 (got.trace, want.trace)):
        assert np.array_equal(a, b)
    assert got.rounds == want.rounds and got.winner == want.winner
    # and uf_table on a program without an application is bound_table
    B2, U2 = RP.uf_table(BC.case(name)[0], T, prog, [])
    assert len(U2) == 0 and np.array_equal(B2.entries, B.entries) and \
        np.array_equal(B2.pieces, B.pieces) and np.array_equal(B2.fixed, B.fixed)


# ---------------------------------------------------------------------------
# uf_probes, uf_table, uf_view
# ---------------------------------------------------------------------------

def _f(arg, name="f", rng=256):
    return N.apply_uf(name, arg.width, rng, arg)


def test_uf_probes_follow_the_destination_rules():
    with N.fresh_scope():
        x, y, t = N.bv_var("x", 256), N.bv_var("y", 256), N.bv_var("t", 256)
        one = _f(N.concat(x, y))
        two = _f(N.bv_op("bvadd", x, y), "g", 64)
        wide = _f(x, "w", 512)                           # range over 256 bits
        deep = _f(N.bv_var("z", 1100), "d")              # domain over 4 chunks
        num = _f(N.bv_num(5, 256), "n")                  # numeral argument
        inside = _f(N.bv_op("bvadd", one, t), "h")       # met under bvadd: not a destination
        cs = [N.bv_cmp("bvult", N.bv_num(9, 256), one),
              N.eq(N.concat(N.extract(63, 0, t), N.zero_extend(128, two)), y),
              N.eq(N.ite(N.bv_cmp("bvult", x, y), num, N.bv_num(0, 256)), t),
              N.eq(N.extract(255, 0, wide), t), N.eq(deep, t), N.eq(one, t),
              N.eq(N.bv_op("bvadd", inside, t), y),
              N.bool_op("not", N.eq(_f(y, "neg"), t))]   # FLAT: no residual is read
        T = RP.distance_trees(cs)
        apps, probes = RP.uf_probes(T)
    assert [a.params[0] for a in apps] == ["f", "g"]     # distinct, first seen
    assert [p.width for p in probes] == [256, 256, 256]  # low chunk first
    assert probes[0].id == y.id and probes[1].id == x.id and probes[2].op == "bvadd"


def test_at_most_64_applications_the_first_ones():
    with N.fresh_scope():
        t = N.bv_var("t", 256)
        cs = [N.eq(_f(N.bv_var("x%02d" % i, 256)), t) for i in range(70)]
        apps, probes = RP.uf_probes(RP.distance_trees(cs))
    assert len(apps) == RP.UF_MAX_SLOTS == len(probes)
    assert [a.args[0].params[0] for a in apps] == ["x%02d" % i for i in range(64)]


def _two_applications():
    """K < f(concat(x, y)) and f(concat(y, x)) = t."""
    x, y, t = N.bv_var("x", 256), N.bv_var("y", 256), N.bv_var("t", 256)
    cs = [N.bv_cmp("bvult", N.bv_num(1 << 200, 256), _f(N.concat(x, y))),
          N.eq(_f(N.concat(y, x)), t)]
    T = RP.distance_trees(cs)
    apps, up = RP.uf_probes(T)
    probes = CS.mask_probes(cs) + CS.mask_probes(T.atom_nodes) + list(T.probes) + list(up)
    return cs, T, apps, up, probes


def test_solve_form_tables_exclude_derived_leaves_and_key_by_probes():
    with N.fresh_scope():
        cs, T, apps, up, probes = _two_applications()
    prog = _compile_search_uncached(cs, probes)
    assert set(prog.entry_keys) == {"f"} and len(prog.entry_keys["f"]) == 2 and prog.derived
    B, U = RP.uf_table(cs, T, prog, apps)
    leaf = {l.name: i for i, l in enumerate(prog.leaves)}
    assert U.n_arg_rows == 4 and U.n_urows == 8 and list(U.keep) == sum(prog.entry_keys["f"], [])
    assert [int(k) for k in U.cands[:, 1]] == [RP.UF_PROBE] * 2          # no else in solve form
    assert U.cands[:, 2:4].tolist() == [[4, 5], [6, 7]]                  # the kept key rows
    for e, name in enumerate(("f#v0#0", "f#v1#0")):      # a derived value leaf is not written
        want = NONE if leaf[name] in prog.derived else leaf[name]
        assert int(U.cands[e, 0]) == want
    assert NONE in U.cands[:, 0].tolist() and any(v != NONE for v in U.cands[:, 0].tolist())
    assert RP.has_slot_piece(B)
    n_user = prog.n_user_probes
    view = RP.uf_view(prog, n_user, U.keep)
    assert view.n_probes == n_user + 4
    outs = lambda p: sorted(int(r[2]) for r in p.code if int(r[0]) & 0xFF == I.OUT)
    assert outs(view) == list(range(n_user + 4)) and len(outs(prog)) == prog.n_probes
    with pytest.raises(ValueError):
        RP.uf_view(prog, n_user, [n_user - 1])


def test_an_argument_probe_equals_its_own_entrys_key_probe():
    """(f) What the PROBE candidates rest on: in solve form application j owns
    entry j, whose key is its own argument under the constructed model, so
    the argument's user probe and the entry's key probe agree on every lane."""
    with N.fresh_scope():
        cs, T, apps, up, probes = _two_applications()
    prog = _compile_search_uncached(cs, probes)
    first = prog.n_user_probes - len(up)
    rng = np.random.default_rng(7)
    for _ in range(64):
        lv = [int.from_bytes(rng.bytes(32), "little") & ((1 << l.width) - 1) for l in prog.leaves]
        _, out = ir_sim.run(prog, lv)
        args = [[out[first + 2 * u + k] for k in range(2)] for u in range(len(apps))]
        keys = [[out[p] for p in key] for key in prog.entry_keys["f"]]
        assert sorted(args) == sorted(keys)
        # each slot finds a candidate whose key is its argument
        assert all(a in keys for a in args)


def test_eval_form_candidates_stand_in_the_tables_order():
    B, U = UC.tables("ckey")
    prog = UC.program("ckey")
    names = [prog.leaves[int(v)].name for v in U.cands[:, 0]]
    assert names == ["f#c0#0", "f#v0#0", "f#v1#0", "f#else#0"]
    assert RP._ints(U.ukeys)[0] == 7 and int(U.cands[0, 2]) == 0
    keys = [[prog.leaves[int(k)].name for k in row[2:3]] for row in U.cands[1:3]]
    assert keys == [["f#k0#0"], ["f#k1#0"]]


def test_the_builder_drops_the_later_slots_until_the_rows_fit():
    with N.fresh_scope():
        t = N.bv_var("t", 256)
        y = N.bv_var("y", 600)                           # 3 chunks with the 8-bit x
        cs = [N.eq(_f(N.concat(N.bv_var("x%02d" % i, 8), y)), t) for i in range(50)]
        T = RP.distance_trees(cs)
        apps, up = RP.uf_probes(T)
        probes = CS.mask_probes(cs) + CS.mask_probes(T.atom_nodes) + list(T.probes) + list(up)
    assert len(apps) == 50 and len(up) == 150
    prog = compile_constraints(cs, probes)
    B, U = RP.uf_table(cs, T, prog, apps)
    assert len(U) == 42 and U.n_urows == U.n_arg_rows == 126 <= RP.UF_MAX_ROWS
    assert [a.id for a in U.apps] == [a.id for a in apps[:42]]
    slots = {int(p) & ~SLOT for p in B.pieces[:, 0] if int(p) & SLOT}
    assert slots == set(range(42))
    why = RP.aim_refusal(apps[45], prog, U)
    assert why and "cap" in why and RP.aim_refusal(apps[3], prog, U) is None


def test_aim_refusal_says_why_an_application_got_no_slot():
    with N.fresh_scope():
        x, t = N.bv_var("x", 256), N.bv_var("t", 256)
        wide, num = _f(x, "w", 512), _f(N.bv_num(5, 256), "n")
        cs = [N.eq(N.extract(255, 0, wide), t), N.eq(num, t), N.eq(_f(x), t)]
        T = RP.distance_trees(cs)
        apps, up = RP.uf_probes(T)
        probes = CS.mask_probes(cs) + CS.mask_probes(T.atom_nodes) + list(T.probes) + list(up)
    prog = compile_constraints(cs, probes)
    _, U = RP.uf_table(cs, T, prog, apps)
    assert "range" in RP.aim_refusal(wide, prog, U)
    assert "constant key" in RP.aim_refusal(num, prog, U)
    assert RP.aim_refusal(apps[0], prog, U) is None
    assert "not a destination" in RP.aim_refusal(apps[0], prog)          # §3.13's answer
    with N.fresh_scope():
        cs2, T2, apps2, up2, probes2 = _two_applications()
    prog2 = _compile_search_uncached(cs2, probes2)
    derived_all = dataclasses.replace(RP.uf_table(cs2, T2, prog2, apps2)[1],
                                      slot_of={}, underived=frozenset(a.id for a in apps2))
    assert "derived" in RP.aim_refusal(apps2[0], prog2, derived_all)


# ---------------------------------------------------------------------------
# the library's resolver and lane function against the specification
# ---------------------------------------------------------------------------

def _row(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u4")


def synthetic(rng):
    """Leaves, a base, U rows and tables that cover every key kind: function 0
    with a two-chunk key (CONST, LEAF, PROBE, ALWAYS candidates, one without a
    value leaf), function 1 with a one-chunk key and 64-bit values (LEAF,
    PROBE, CONST); keys and arguments are small numbers, so they meet."""
    gens = [LeafGen(256, 0, 0, 0, 0, 0) for _ in range(10)] + \
        [LeafGen(64, 0, 0, 0, 0, 0) for _ in range(4)]
    small = lambda: int(rng.integers(0, 3))
    base = np.stack([_row(small()) if rng.integers(0, 2) else
                     _row(int.from_bytes(rng.bytes(32 if i < 10 else 8), "little"))
                     for i in range(14)]).astype(np.uint32)
    urows = np.stack([_row(small()) for _ in range(6)]).astype(np.uint32)
    U = RP.make_ufs(slots=[(0, 0), (0, 2), (1, 4), (1, 5)], funcs=[(0, 4, 2), (4, 3, 1)],
                    cands=[(0, RP.UF_CONST, 0, 1, 0, 0), (NONE, RP.UF_LEAF, 4, 5, 0, 0),
                           (2, RP.UF_PROBE, 2, 3, 0, 0), (3, RP.UF_ALWAYS, 0, 0, 0, 0),
                           (10, RP.UF_LEAF, 6, 0, 0, 0), (11, RP.UF_PROBE, 0, 0, 0, 0),
                           (12, RP.UF_CONST, 2, 0, 0, 0)], ukeys=[0, 1, 2], n_urows=6)
    B = RP.make_bounds([(0, [(SLOT | 0, 0, 0, 256)]),
                        (1, [(SLOT | 2, 0, 0, 64)], RP.BOUND_HIGH_STRICT, 1, 0),
                        (2, [(SLOT | 1, 8, 0, 100), (5, 0, 100, 50)], RP.BOUND_LOW, 0, 7),
                        (1, [(SLOT | 3, 0, 3, 20), (13, 3, 30, 9)]),
                        (0, [(7, 0, 0, 256)], RP.BOUND_HIGH, RP.BOUND_ATOM | 1, 0)], 2, 3)
    rv = np.stack([_row(int.from_bytes(rng.bytes(32), "little")) for _ in range(3)])
    return gens, base, urows, U, B, rv.astype(np.uint32)


def test_library_resolver_and_lanes_equal_the_specification_on_synthetic_tables():
    rng = np.random.default_rng(0x7566)
    consts = np.zeros((1, 8), dtype=np.uint32)
    seen, aimed = set(), 0
    for it in range(40):
        gens, base, urows, U, B, rv = synthetic(rng)
        want = RP.uf_resolve_ref(base, urows, U)
        got = walk_uf_resolve_host(gens, base, urows, U)
        assert np.array_equal(want, got)
        seen |= set(want.tolist())
        state = (rv, np.array([0, rng.integers(0, 2)], bool),
                 np.array([1, rng.integers(0, 2), 0], bool), want)
        for r, lanes in ((0, 64), (1, 16), (5, 257)):
            spec = RP.uf_mutate_ref(gens, consts, base, state, B, 77, r, lanes)
            lib, moves = walk_uf_mutate_host(gens, consts, base, state, B, U, 77, r, lanes)
            assert np.array_equal(spec, lib)
            picks = RP.uf_picks_ref(state, B, r, lanes)
            assert np.array_equal(moves[:, 4].astype(np.int64), picks)
            aimed += int((picks != NONE).sum())
        # round 0: nothing is known, every lane is the plain walk's
        spec = RP.uf_mutate_ref(gens, consts, base, None, B, 77, 0, 64)
        lib, moves = walk_uf_mutate_host(gens, consts, base, None, B, U, 77, 0, 64)
        assert np.array_equal(spec, lib) and (moves[:, 4] == NONE).all()
    # every candidate kind was hit, and a slot was left unresolved
    assert {0, 2, 3, 10, 11, 12, NONE} <= seen and aimed > 100


@pytest.mark.parametrize("name", UC.NAMES)
def test_library_equals_the_specification_on_the_cases(name):
    prog = UC.program(name)
    B, U = UC.tables(name)
    gens, consts = default_leafgen(prog), UC.consts_of(prog)
    res = UC.reference(name)
    for base in (UC.start_rows(name), np.asarray(res.leaves[0])):
        bits, abits, resid, urows = UC.values_fn(name)(np.ascontiguousarray(base[:, :, None]))
        want = RP.uf_resolve_ref(base, urows[:, :, 0], U)
        assert np.array_equal(walk_uf_resolve_host(gens, base, urows[:, :, 0], U), want)
        state = (resid[:, :, 0], bits[0], abits[0], want)
        for r, lanes in ((1, 16), (2, 300)):
            spec = RP.uf_mutate_ref(gens, consts, base, state, B, UC.SEED, r, lanes)
            lib, _ = walk_uf_mutate_host(gens, consts, base, state, B, U, UC.SEED, r, lanes)
            assert np.array_equal(spec, lib)


def test_with_no_slot_piece_it_is_the_lane_function_of_bounds():
    name = "fixed"
    prog, B = BC.program(name), BC.bounds(name)
    gens, consts = default_leafgen(prog), BC.consts_of(prog)
    base = BC.start_rows(name)
    bits, abits, resid = BC.values_fn(name)(np.ascontiguousarray(base[:, :, None]))
    state = (resid[:, :, 0], bits[0], abits[0])
    for r, lanes in ((1, 64), (3, 257)):
        want, wm = walk_bound_mutate_host(gens, consts, base, state, B, 5, r, lanes)
        got, gm = walk_uf_mutate_host(gens, consts, base, state + (np.zeros(0, np.uint32),), B,
                                      RP.no_ufs(), 5, r, lanes)
        assert np.array_equal(want, got) and np.array_equal(wm, gm)
        assert np.array_equal(RP.uf_mutate_ref(gens, consts, base, state + ([],), B, 5, r, lanes),
                              RP.bound_mutate_ref(gens, consts, base, state, B, 5, r, lanes))


# ---------------------------------------------------------------------------
# the validator
# ---------------------------------------------------------------------------

def _refused(gens, base, urows, U, B=None, state=None):
    with pytest.raises(EngineError):
        if B is None:
            walk_uf_resolve_host(gens, base, urows, U)
        else:
            walk_uf_mutate_host(gens, np.zeros((1, 8), np.uint32), base, state, B, U, 1, 1, 64)


def test_malformed_uf_tables_are_refused():
    rng = np.random.default_rng(1)
    gens, base, urows, U, B, rv = synthetic(rng)
    walk_uf_resolve_host(gens, base, urows, U)           # the table itself is accepted

    def changed(table, row, col, value):
        a = np.array(getattr(U, table), dtype=np.uint32, copy=True)
        a[row, col] = value
        return dataclasses.replace(U, **{table: a})
    bad = [changed("slots", 0, 0, 2),                    # function index
           changed("slots", 1, 1, 5),                    # a two-chunk argument from the last row
           changed("slots", 3, 1, 6),                    # argument row at n_urows
           changed("funcs", 0, 2, 0), changed("funcs", 0, 2, 5),         # chunks 1 .. 4
           changed("funcs", 1, 1, 4),                    # candidates past the table
           changed("funcs", 1, 0, 8),
           changed("cands", 0, 0, 14),                   # value leaf
           changed("cands", 0, 1, 4),                    # key kind
           changed("cands", 0, 3, 3),                    # CONST row at n_ukeys
           changed("cands", 1, 2, 14),                   # LEAF key
           changed("cands", 2, 3, 6),                    # PROBE row at n_urows
           changed("cands", 4, 0, 0),                    # value leaves of 64 and 256 bits
           dataclasses.replace(U, n_urows=5),            # rows the tables reach past
           dataclasses.replace(U, n_urows=RP.UF_MAX_ROWS + 1)]
    for u in bad:
        _refused(gens, base, np.zeros((RP.UF_MAX_ROWS + 1, 8), np.uint32), u)
    # unread words are not checked: a key word past the function's chunks, an ALWAYS key
    walk_uf_resolve_host(gens, base, urows, changed("cands", 4, 3, 999))
    walk_uf_resolve_host(gens, base, urows, changed("cands", 3, 2, 999))
    # the caps
    many = RP.make_ufs(slots=[(0, 0)] * 65, funcs=[(0, 1, 1)], cands=[(0, RP.UF_ALWAYS, 0, 0, 0, 0)],
                       n_urows=1)
    _refused(gens, base, urows, many)
    walk_uf_resolve_host(gens, base, urows, dataclasses.replace(many, slots=many.slots[:64]))
    _refused(gens, base, urows, RP.make_ufs(funcs=[(0, 257, 1)],
                                            cands=[(0, RP.UF_ALWAYS, 0, 0, 0, 0)] * 257, n_urows=1))


def test_malformed_slot_pieces_are_refused():
    rng = np.random.default_rng(2)
    gens, base, urows, U, B, rv = synthetic(rng)
    state = (rv, np.zeros(2, bool), np.zeros(3, bool), RP.uf_resolve_ref(base, urows, U))
    walk_uf_mutate_host(gens, np.zeros((1, 8), np.uint32), base, state, B, U, 1, 1, 64)
    for pieces in ([(SLOT | 4, 0, 0, 8)],                # slot index
                   [(SLOT | 2, 60, 0, 8)],               # past the function's 64-bit values
                   [(SLOT | 2, 0, 0, 65)],
                   [(SLOT | 0, 0, 250, 8)],              # past the residual
                   [(SLOT | 0, 0, 0, 0)]):
        _refused(gens, base, urows, U, RP.make_bounds([(0, pieces)], 2, 3), state)
    # the edges are accepted
    ok = RP.make_bounds([(0, [(SLOT | 2, 0, 0, 64), (SLOT | 3, 63, 255, 1), (SLOT | 0, 0, 0, 256)])],
                        2, 3)
    walk_uf_mutate_host(gens, np.zeros((1, 8), np.uint32), base, state, ok, U, 1, 1, 64)
    # a function without any value leaf gives its slots no width
    none = dataclasses.replace(U, cands=np.array(
        [[NONE] + row[1:] for row in U.cands.tolist()], dtype=np.uint32))
    _refused(gens, base, urows, none, B, state)
    # a destination that is neither a leaf nor none
    _refused(gens, base, urows, U, B, state[:3] + (np.array([14, 0, 0, 0], np.uint32),))


def test_null_tables_with_counts_are_refused():
    import ctypes as C
    from mythril_amd.engine import load_library
    lib = load_library()
    rng = np.random.default_rng(3)
    gens, base, urows, U, B, rv = synthetic(rng)
    garr = (LeafGen * len(gens))(*gens)
    p = lambda a: np.ascontiguousarray(a, dtype=np.uint32).ctypes.data_as(C.c_void_p)
    dest = np.zeros(4, dtype=np.uint32)
    full = [C.cast(garr, C.c_void_p), len(gens), p(base), p(urows), 6, p(U.slots), 4, p(U.funcs), 2,
            p(U.cands), 7, p(U.ukeys), 3, p(dest)]
    assert lib.mg_walk_uf_resolve_host(*full) == 0
    for k in (0, 2, 3, 5, 7, 9, 11, 13):
        q = list(full)
        q[k] = None
        assert lib.mg_walk_uf_resolve_host(*q) == -1

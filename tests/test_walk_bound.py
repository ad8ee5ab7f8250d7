"""CPU tests of the walk with aims for orders: the table's
order, strictness, cap and dropped sides, an applied order entry against
Python ints and the oracle (oracle/smtlib_ref.py), the library's lane function
(csrc/mg_walk_bound.h through mg_walk_bound_mutate_host) against its
specification ``repair.bound_mutate_ref`` limb for limb, the validator's
refusals, and the conditions on the crafted cases of tests/bound_cases.py.  No
GPU."""

import dataclasses

import numpy as np
import pytest

import bound_cases as BC
from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import (EngineError, LeafGen, default_leafgen, repair_mutate_host,
                                walk_aim_mutate_host, walk_bound_mutate_host)
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N
from oracle import smtlib_ref as R

NONE = RP.AIM_NONE
M256 = (1 << 256) - 1
LOW, LOW_S, HIGH, HIGH_S = (RP.BOUND_LOW, RP.BOUND_LOW_STRICT, RP.BOUND_HIGH,
                            RP.BOUND_HIGH_STRICT)


# ---------------------------------------------------------------------------
# the crafted cases
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", BC.NAMES)
def test_crafted_cases_need_the_order_aims(name):
    """The conditions on the inputs, none of them a measurement: (a) the
    generator finds no model among lanes x max_rounds candidates, (b) walk_ref
    with the tree scoring and the aim table of §3.12 is still failing after
    max_rounds from the same start, (c) with the table of §3.13 it reaches a
    model within half of max_rounds."""
    rounds = BC.MAX_ROUNDS[name]
    T, B = BC.trees(name), BC.bounds(name)
    assert len(BC.aims(name)) == 0                       # no equality: nothing §3.12 can aim
    assert [int(m) for m in B.entries[:, 3]] == {
        "window": [LOW, HIGH, LOW], "signed": [HIGH_S, LOW], "fixed": [HIGH_S, LOW]}[name]
    assert [int(t) for t in B.entries[:, 4]] == {"window": [0, 0, 1]}.get(name, [0, 1])
    assert [len(B.of(e)) for e in range(len(B))] == {
        "window": [1, 32, 32], "signed": [3, 3], "fixed": [31, 31]}[name]
    assert [B.fixed_of(e) for e in range(len(B))] == {"fixed": [0x80, 0x80]}.get(
        name, [0] * len(B))
    if name == "signed":                                 # no edge on a multiple of 32
        assert [p[1:] for p in B.of(0)] == [(0, 156, 100), (0, 143, 13), (0, 0, 143)]
        assert not T.is_tree(1) and T.kind(1) == RP.MAGNITUDE      # the converted negation
    if name == "fixed":                                  # the fixed bits sit below the pieces
        assert min(p[2] for p in B.of(0)) == 8
    start = BC.start_rows(name)
    bits = BC.values_fn(name)(start[:, :, None])[0][0]
    assert (~bits).sum() == 1                            # one root short of a model
    assert BC.generator_hits(name, BC.LANES * rounds) == 0                        # (a)
    stuck = BC.reference(name, bound=False)
    assert stuck.nfail[0] > 0 and stuck.rounds == rounds                          # (b)
    res = BC.reference(name)
    zero = np.flatnonzero(res.trace[0, :res.rounds, 0] == 0)
    assert zero.size and int(zero[0]) < rounds // 2                               # (c)
    assert int(zero[0]) == BC.FIRST_ZERO[name]           # what the cases' docstring says
    assert res.nfail[0] == 0 == res.cost[0] and res.winner == 0 and res.rounds % 8 == 0
    assert BC.values_fn(name)(np.asarray(res.leaves[0])[:, :, None])[0].all()


def test_walk_ref_with_xor_entries_only_is_the_aimed_walk():
    import aim_cases as AC
    name = "odd"
    prog, T, A = AC.program(name), AC.trees(name), AC.aims(name)
    want = AC.reference(name, 2, 256, 8)
    got = RP.walk_ref(AC.values_fn(name), default_leafgen(prog), AC.consts_of(prog),
                      AC.starts(name, 2), T.roots, AC.SEED, 256, 8, 8, score=RP.tree_scoring(T),
                      bounds=RP.bounds_of_aims(A, len(T.roots), T.n_atoms))
    for a, b in ((got.leaves, want.leaves), (got.nfail, want.nfail), (got.cost, want.cost),
                 (got.trace, want.trace)):
        assert np.array_equal(a, b)
    assert got.rounds == want.rounds and got.winner == want.winner


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def orders():
    """Roots: an equality (two XOR entries), a tree with a strict and a lax
    atom over one probe's operands and an equality, simple orders of every
    operator, a negated one, one whose sides do not resolve, one with a
    numeral side and one over 65 one-bit leaves."""
    with N.fresh_scope():
        v = lambda s, w=16: N.bv_var(s, w)
        a, b, c, d, e, f = (v(s) for s in "abcdef")
        mul = N.bv_op("bvmul", v("m"), v("n"))
        bits65 = N.concat(*[v("o%02d" % k, 1) for k in range(65)])
        cs = [N.eq(a, b),
              N.bool_op("or", N.bool_op("and", N.bv_cmp("bvult", c, d), N.eq(e, f)),
                        N.bv_cmp("bvule", c, d)),
              N.bv_cmp("bvugt", a, c),                   # lo = c, hi = a, strict
              N.bv_cmp("bvsge", b, d),                   # lo = d, hi = b
              N.bool_op("not", N.bv_cmp("bvslt", e, f)),  # bvsge(e, f): lo = f, hi = e
              N.bv_cmp("bvule", mul, N.bv_op("bvadd", a, b)),         # neither side
              N.bv_cmp("bvult", N.bv_num(9, 16), f),     # a numeral has no piece
              N.bv_cmp("bvsle", N.concat(v("g", 8), N.bv_num(0x5A, 8)), mul),
              N.bv_cmp("bvult", bits65, v("w", 65))]     # 65 pieces: dropped; w resolves
        T = RP.distance_trees(cs)
        prog = compile_constraints(cs, CS.mask_probes(cs) + CS.mask_probes(T.atom_nodes)
                                   + list(T.probes))
    return cs, T, prog


def test_the_table_is_ordered_xor_then_atoms_then_roots(orders):
    cs, T, prog = orders
    B = RP.bound_table(cs, T, prog)                      # outside the scope of the nodes
    A = RP.aim_table(T, prog)
    n = len(A)
    assert n >= 2 and np.array_equal(B.entries[:n, :3], A.entries) and B.pieces[:len(A.pieces)].tolist() \
        == A.pieces.tolist()
    assert (B.entries[:n, 3:] == 0).all() and not B.fixed[:n].any() and B.sides[:n] == A.sides
    rest = [tuple(int(x) for x in row) for row in B.entries[n:]]
    modes, truth = [r[3] for r in rest], [r[4] for r in rest]
    atoms = [i for i, e in enumerate(T.atoms) if int(e) >> 16 == RP.MAGNITUDE]
    assert len(atoms) == 2 and T.is_tree(1)
    # two atoms share the operands (one probe) with different strictness
    strict = T.atom_nodes[atoms[0]].op == "bvult"
    first = [LOW_S, HIGH_S] if strict else [LOW, HIGH]
    second = [LOW, HIGH] if strict else [LOW_S, HIGH_S]
    assert modes[:4] == first + second
    assert truth[:4] == [RP.BOUND_ATOM | atoms[0]] * 2 + [RP.BOUND_ATOM | atoms[1]] * 2
    assert rest[0][0] == rest[1][0] == rest[2][0] == rest[3][0]
    # then the simple roots, in root order
    assert modes[4:] == [LOW_S, HIGH_S, LOW, HIGH, LOW, HIGH, HIGH_S, LOW, HIGH_S]
    assert truth[4:] == [2, 2, 3, 3, 4, 4, 6, 7, 8]
    leaf = {l.source: i for i, l in enumerate(prog.leaves)}
    side = lambda k: B.of(n + k)[0][0]
    assert (side(4), side(5)) == (leaf["c"], leaf["a"])               # bvugt(a, c)
    assert (side(6), side(7)) == (leaf["d"], leaf["b"])               # bvsge(b, d)
    assert (side(8), side(9)) == (leaf["f"], leaf["e"])               # not bvslt(e, f)
    assert side(10) == leaf["f"] and side(12) == leaf["w"]
    assert B.of(n + 11) == [(leaf["g"], 0, 8, 8)] and B.fixed_of(n + 11) == 0x5A
    assert all(B.fixed_of(n + k) == 0 for k in range(len(rest)) if k != 11)
    # every probe is the bvsub of the side's operands
    for k, r in enumerate(rest):
        assert T.probes[r[0]].op == "bvsub"
    assert B.n_roots == len(cs) and B.n_atoms == T.n_atoms and B.n_order == len(rest)
    # a derived leaf drops the side, not the entry of the other side
    derived = dataclasses.replace(prog, derived={leaf["c"]: 0})
    D = RP.bound_table(cs, T, derived)
    assert D.n_order == B.n_order - 3                    # c: two atom entries and root 2's lo


def test_at_most_256_entries_the_first_ones():
    with N.fresh_scope():
        cs = [N.bv_cmp("bvult", N.bv_var("x%03d" % k, 8), N.bv_var("y%03d" % k, 8))
              for k in range(130)]
        cs[0] = N.eq(N.bv_var("x000", 8), N.bv_var("y000", 8))
        T = RP.distance_trees(cs)
        prog = compile_constraints(cs, CS.mask_probes(cs) + list(T.probes))
    B = RP.bound_table(cs, T, prog)
    assert len(B) == 256 == RP.AIM_MAX_ENTRIES and len(B.sides) == 256
    assert [int(m) for m in B.entries[:, 3]] == [0, 0] + [LOW_S, HIGH_S] * 127
    assert [int(t) for t in B.entries[2:, 4]] == [1 + k // 2 for k in range(254)]


def test_a_root_that_fell_back_to_classify_gets_no_entry(monkeypatch):
    with N.fresh_scope():
        a, b, c, d = (N.bv_var(s, 16) for s in "abcd")
        cs = [N.bool_op("or", N.bv_cmp("bvult", a, b), N.bv_cmp("bvult", c, d)),
              N.bv_cmp("bvult", a, c)]
        monkeypatch.setattr(RP, "MAX_ATOMS", 1)
        T = RP.distance_trees(cs)
        monkeypatch.undo()
        prog = compile_constraints(cs, CS.mask_probes(cs) + CS.mask_probes(T.atom_nodes)
                                   + list(T.probes))
    assert not T.is_tree(0) and T.kind(0) == RP.MAGNITUDE and T.n_atoms == 0     # the fallback
    B = RP.bound_table(cs, T, prog)
    assert [int(t) for t in B.entries[:, 4]] == [1, 1]


# ---------------------------------------------------------------------------
# an applied entry: Python ints and the oracle
# ---------------------------------------------------------------------------

def _state(name, base):
    vals = BC.values_fn(name)(np.ascontiguousarray(base[:, :, None]))
    return np.ascontiguousarray(vals[2][:, :, 0]), vals[0][0], vals[1][0]


def _side_value(B, e, rows):
    vals = RP._ints(rows)
    v = B.fixed_of(e)
    for leaf, leaf_bit, value_bit, n in B.of(e):
        v |= (vals[leaf] >> leaf_bit & ((1 << n) - 1)) << value_bit
    return v


@pytest.mark.parametrize("name", BC.NAMES)
def test_an_applied_order_entry_lands_on_the_other_side(name):
    """Every entry of the crafted cases covers its side (pieces and fixed), so
    the applied lane's side is hi - s, respectively lo + s, where the
    scattered bits can hold it (`fixed`: up to the numeral byte)."""
    prog, B, T = BC.program(name), BC.bounds(name), BC.trees(name)
    gens, consts = default_leafgen(prog), BC.consts_of(prog)
    cs = BC.case(name)[0]
    rng = np.random.default_rng(5)
    seen = 0
    for _ in range(6):
        base = BC.start_rows(name).copy()
        for leaf, l in enumerate(prog.leaves):           # any assignment at all
            v = int.from_bytes(rng.bytes(32), "little") & ((1 << l.width) - 1)
            base[leaf] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
        state = _state(name, base)
        live = RP.bound_live_ref(state, B)
        assert live == [e for e in range(len(B)) if not state[1][int(B.entries[e, 4])]]
        out, moves = walk_bound_mutate_host(gens, consts, base, state, B, 3, 1, 64,
                                            n_resid=T.n_resid)
        assert np.array_equal(out, RP.bound_mutate_ref(gens, consts, base, state, B, 3, 1, 64))
        for j in range(1, len(live) + 1):
            e = int(moves[j, 4])
            assert e == live[(j - 1 + len(live)) % len(live)] and moves[j, 0] == 0
            p, _, _, mode, k = (int(x) for x in B.entries[e])
            D = RP._ints(state[0][p:p + 1])[0]
            V = _side_value(B, e, base)
            s = 1 if mode in (LOW_S, HIGH_S) else 0
            # D = lo - hi: the other side is V - D (LOW: hi) or V + D (HIGH: lo)
            want = (V - D - s if mode <= LOW_S else V + D + s) & M256
            got = _side_value(B, e, out[:, :, j])
            keep = M256 ^ 0xFF if name == "fixed" else M256
            assert got & keep == want & keep and got & ~keep == V & ~keep
            other = [l for l in range(len(base)) if l not in {q[0] for q in B.of(e)}]
            assert np.array_equal(out[other, :, j], base[other])
            if name != "fixed":                          # the root then holds in the oracle
                rows = out[:, :, j]
                assert BC.values_fn(name)(np.ascontiguousarray(rows[:, :, None]))[0][0][k]
            seen += 1
    assert seen >= 6


# ---------------------------------------------------------------------------
# the lane function: the library against the specification
# ---------------------------------------------------------------------------

WIDTHS = (256, 100, 13, 143, 8, 64, 33)
N_RESID, N_ROOTS, N_ATOMS = 48, 300, 70


def synthetic(seed, n_entries, xor_only=False):
    """(leafgen, consts, base, state, bounds): seven leaves, entry 0 of one
    piece across limbs, entry 1 of 64, the others of 1 .. 6 pieces anywhere
    inside their leaves and the value, every mode, truth bits over two root
    mask probes and three atom mask words; a third of the residuals zero, half
    of the truth bits clear."""
    rng = np.random.default_rng(seed)
    consts = rng.integers(0, 1 << 32, size=(6, 8), dtype=np.uint64).astype(np.uint32)
    gens = [LeafGen(w, 2 * (i % 2), 3 * (i % 2), 50, 70, 85) for i, w in enumerate(WIDTHS)]
    base = rng.integers(0, 1 << 32, size=(len(WIDTHS), 8), dtype=np.uint64).astype(np.uint32)
    for i, w in enumerate(WIDTHS):
        v = RP._ints(base[i:i + 1])[0] & ((1 << w) - 1)
        base[i] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    rvals = rng.integers(0, 1 << 32, size=(N_RESID, 8), dtype=np.uint64).astype(np.uint32)
    rvals[rng.integers(0, 3, size=N_RESID) == 0] = 0
    rvals[:2] |= 1
    rbits, abits = rng.integers(0, 2, size=N_ROOTS) == 1, rng.integers(0, 2, size=N_ATOMS) == 1

    def piece():
        leaf = int(rng.integers(len(WIDTHS)))
        n = 1 + int(rng.integers(WIDTHS[leaf]))
        return (leaf, int(rng.integers(WIDTHS[leaf] - n + 1)), int(rng.integers(256 - n + 1)), n)
    entries = []
    for e in range(n_entries):
        cnt = 1 if e == 0 else 64 if e == 1 else 1 + int(rng.integers(6))
        ps = [piece() for _ in range(cnt)]
        if e == 0:
            ps = [(0, 17, 5, 200)]                       # crosses limbs on both sides
        mode = 0 if xor_only else (e + 1) % 5
        if mode == 0:
            entries.append((e % N_RESID, ps))
            continue
        truth = (RP.BOUND_ATOM | int(rng.integers(N_ATOMS))) if e % 2 else int(rng.integers(N_ROOTS))
        if e < 2:
            truth = (255, RP.BOUND_ATOM | 64)[e]         # live below
        entries.append((e % N_RESID, ps, mode, truth, int.from_bytes(rng.bytes(32), "little")))
    rbits[255], abits[64] = False, False
    return gens, consts, base, (rvals, rbits, abits), RP.make_bounds(entries, N_ROOTS, N_ATOMS)


@pytest.mark.parametrize("lanes", [1, 7, 8, 16, 63, 4096])
@pytest.mark.parametrize("n_entries", [0, 1, 5, 40])
def test_library_lanes_equal_the_specification(lanes, n_entries):
    gens, consts, base, state, B = synthetic(lanes * 64 + n_entries, n_entries)
    live = RP.bound_live_ref(state, B)
    cap = lanes // 8
    n1 = min(len(live), cap)
    landed = 0
    for r, st in ((0, None), (0, state), (3, state), (65535, state)):
        want = RP.bound_mutate_ref(gens, consts, base, st, B, 0xB0B, r, lanes)
        got, moves = walk_bound_mutate_host(gens, consts, base, st, B, 0xB0B, r, lanes,
                                            n_resid=N_RESID)
        assert np.array_equal(got, want)
        picks = RP.bound_picks_ref(st, B, r, lanes)
        assert np.array_equal(moves[:, 4].astype(np.int64), picks)
        plain, pmoves = repair_mutate_host(gens, consts, base, 0xB0B, r, lanes)
        if st is None:                                   # round 0: today's neighbours
            assert (picks == NONE).all() and np.array_equal(got, plain)
            continue
        assert (picks != NONE).sum() == 2 * n1
        assert np.array_equal(got[:, :, 2 * n1 + 1:], plain[:, :, 2 * n1 + 1:])
        assert np.array_equal(got[:, :, 0], base)
        assert (moves[1:n1 + 1, 0] == 0).all()                      # the entry and nothing else
        assert np.array_equal(moves[n1 + 1:, :4], pmoves[n1 + 1:])
        if n1:                                           # the rotation
            assert picks[1] == live[(r * n1) % len(live)] == picks[n1 + 1]
            assert picks[n1] == live[(n1 - 1 + r * n1) % len(live)] == picks[2 * n1]
        for j in range(n1 + 1, 2 * n1 + 1):              # a plain move on an aimed leaf wins
            for m in range(int(moves[j, 0])):
                leaf = int(moves[j, 2 + m])
                if leaf in {p[0] for p in B.of(int(picks[j]))} and \
                        (m + 1 == int(moves[j, 0]) or int(moves[j, 3]) != leaf):
                    landed += 1
                    assert np.array_equal(got[leaf, :, j], plain[leaf, :, j])
    if n_entries >= 5 and lanes >= 63:
        assert landed > 0
    if n_entries == 40 and 8 <= lanes <= 63:
        assert len(live) > cap                           # above the cap: the list rotates
    if n_entries >= 1:
        assert 0 in live                                 # truth bit 255: the second root word row


def test_lane_ranges_of_the_host_entry():
    gens, consts, base, state, B = synthetic(7, 12)
    whole, moves = walk_bound_mutate_host(gens, consts, base, state, B, 9, 2, 300, n_resid=N_RESID)
    part, pm = walk_bound_mutate_host(gens, consts, base, state, B, 9, 2, 300, lane0=5,
                                      n_lanes=60, n_resid=N_RESID)
    assert np.array_equal(part, whole[:, :, 5:65]) and np.array_equal(pm, moves[5:65])


@pytest.mark.parametrize("lanes", [1, 16, 64, 1000])
def test_with_no_order_entry_it_is_the_aimed_lane_function(lanes):
    gens, consts, base, state, B = synthetic(11, 20, xor_only=True)
    assert B.n_order == 0 and len(B) == 20
    A = RP.Aims(np.ascontiguousarray(B.entries[:, :3]), B.pieces, [0] * len(B))
    for r, st in ((0, None), (1, state), (9, state)):
        rv = None if st is None else st[0]
        want = RP.aim_mutate_ref(gens, consts, base, rv, A, 77, r, lanes)
        assert np.array_equal(RP.bound_mutate_ref(gens, consts, base, st, B, 77, r, lanes), want)
        assert np.array_equal(RP.bound_picks_ref(st, B, r, lanes),
                              RP.aim_picks_ref(rv, A, r, lanes))
        got, gm = walk_bound_mutate_host(gens, consts, base, st, B, 77, r, lanes, n_resid=N_RESID)
        lib, lm = walk_aim_mutate_host(gens, consts, base, rv, A, 77, r, lanes, n_resid=N_RESID)
        assert np.array_equal(got, want) and np.array_equal(got, lib) and np.array_equal(gm, lm)


ONE = [(0, 0, 0, 1)]
MALFORMED = {
    "residual index at n_resid": [(N_RESID, [(0, 0, 0, 8)])],
    "an entry without pieces": [(0, [])],
    "65 pieces": [(0, [(4, 0, 0, 1)] * 65, LOW, 0, 0)],
    "leaf at n_leaves": [(0, [(len(WIDTHS), 0, 0, 1)], HIGH, 0, 0)],
    "leaf_bit + len above the width": [(0, [(2, 6, 0, 8)])],
    "leaf_bit above the width": [(0, [(2, 14, 0, 1)])],
    "value_bit + len above 256": [(0, [(0, 0, 250, 7)], LOW_S, 0, 0)],
    "value_bit above 256": [(0, [(0, 0, 300, 1)])],
    "len 0": [(0, [(0, 0, 0, 0)])],
    "len above 256": [(0, [(0, 0, 0, 257)])],
    "257 entries": [(0, ONE)] * 257,
    "mode 5": [(0, ONE, 5, 0, 0)],
    "a root truth at n_roots": [(0, ONE, LOW, N_ROOTS, 0)],
    "an atom truth at n_atoms": [(0, ONE, HIGH_S, RP.BOUND_ATOM | N_ATOMS, 0)],
    "an XOR entry with a truth": [(0, ONE, 0, 3, 0)],
    "an XOR entry with an atom truth": [(0, ONE, 0, RP.BOUND_ATOM, 0)],
    "an XOR entry with fixed bits": [(0, ONE, 0, 0, 1 << 255)],
}


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_malformed_tables_are_refused(kind):
    gens, consts, base, state, _ = synthetic(1, 0)
    with pytest.raises(EngineError):
        walk_bound_mutate_host(gens, consts, base, state,
                               RP.make_bounds(MALFORMED[kind], N_ROOTS, N_ATOMS), 1, 1, 64,
                               n_resid=N_RESID)


def test_the_edges_of_the_validator_are_accepted():
    gens, consts, base, state, _ = synthetic(1, 0)
    ok = RP.make_bounds([(N_RESID - 1, [(2, 5, 248, 8)], HIGH_S, N_ROOTS - 1, M256),
                         (0, [(4, 0, 0, 1)] * 64, LOW, RP.BOUND_ATOM | (N_ATOMS - 1), 0)],
                        N_ROOTS, N_ATOMS)
    walk_bound_mutate_host(gens, consts, base, state, ok, 1, 1, 64, n_resid=N_RESID)


def test_pieces_outside_the_piece_array_are_refused():
    gens, consts, base, state, _ = synthetic(1, 0)
    ok = RP.make_bounds([(0, [(0, 0, 0, 8), (1, 0, 8, 8)], LOW, 0, 0)], N_ROOTS, N_ATOMS)
    walk_bound_mutate_host(gens, consts, base, state, ok, 1, 1, 64, n_resid=N_RESID)
    for off, cnt in ((1, 2), (2, 1), (3, 1), (0xFFFFFFFF, 2), (0, 3)):
        bad = dataclasses.replace(ok, entries=np.array([[0, off, cnt, LOW, 0]], dtype=np.uint32))
        with pytest.raises(EngineError):
            walk_bound_mutate_host(gens, consts, base, state, bad, 1, 1, 64, n_resid=N_RESID)


def test_null_tables_with_counts_are_refused():
    import ctypes as C
    from mythril_amd.engine import load_library
    lib = load_library()
    gens, consts, base, state, B = synthetic(2, 3)
    garr = (LeafGen * len(gens))(*gens)
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    mvals = np.concatenate([RP.bound_mask_words(state[1]), RP.bound_mask_words(state[2])])
    assert mvals.shape == (16 + 8,)
    out = np.zeros((len(gens), 8, 64), dtype=np.uint32)
    full = [C.cast(garr, C.c_void_p), len(gens), p(consts), len(consts), p(base), p(state[0]),
            N_RESID, p(mvals), N_ROOTS, N_ATOMS, p(B.entries), len(B), p(B.pieces), len(B.pieces),
            p(B.fixed), 1, 1, 64, 0, 64, p(out), None]
    assert lib.mg_walk_bound_mutate_host(*full) == 0
    for k in (10, 12, 14):
        q = list(full)
        q[k] = None
        assert lib.mg_walk_bound_mutate_host(*q) == -1

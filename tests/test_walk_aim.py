"""CPU tests of the aimed walk: the aim table's resolution
rules against the oracle (oracle/smtlib_ref.py), the library's lane function
(csrc/mg_walk_aim.h through mg_walk_aim_mutate_host) against its specification
``repair.aim_mutate_ref`` limb for limb, the validator's refusals, and the
conditions on the crafted cases of tests/aim_cases.py.  No GPU."""

import dataclasses
import types

import numpy as np
import pytest

import aim_cases as AC
import tree_cases as TC
from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import (EngineError, LeafGen, default_leafgen, repair_mutate_host,
                                walk_aim_mutate_host)
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N
from oracle import smtlib_ref as R

NONE = RP.AIM_NONE


# ---------------------------------------------------------------------------
# the crafted cases
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", AC.NAMES)
def test_crafted_cases_need_the_aim(name):
    """The conditions on the inputs, none of them a measurement: (a) the
    generator finds no model among lanes x max_rounds candidates, (b) walk_ref
    with the tree scoring and no aims is still failing after max_rounds from
    the same start, (c) with aims it reaches a model within half of
    max_rounds."""
    rounds = AC.MAX_ROUNDS[name]
    T, A = AC.trees(name), AC.aims(name)
    assert len(A) == {"bytes": 2, "wide": 4, "odd": 1}[name]
    assert sorted(len(A.of(e)) for e in range(len(A))) == {
        "bytes": [1, 32], "wide": [1, 1, 2, 2], "odd": [3]}[name]
    if name == "wide":                                   # the chunks cut a_mid at bit 128
        assert sorted(p[1] for e in range(len(A)) for p in A.of(e))[-1] == 128
    if name == "odd":                                    # no edge on a multiple of 32
        assert not T.is_tree(0) and T.kind(0) == RP.HAMMING
        assert [p[1:] for p in A.of(0)] == [(0, 156, 100), (0, 143, 13), (0, 0, 143)]
    start = AC.start_rows(name)
    bits = AC.values_fn(name)(start[:, :, None])[0][0]
    assert (~bits).sum() == 1                            # one root short of a model
    assert AC.generator_hits(name, AC.LANES * rounds) == 0                        # (a)
    stuck = AC.reference(name, aimed=False)
    assert stuck.nfail[0] > 0 and stuck.rounds == rounds                          # (b)
    assert (stuck.trace[0, :, 0] == stuck.trace[0, 0, 0]).all()   # the count never improves
    assert stuck.cost[0] >= AC.BLOCK                     # the coupled block is what is left
    res = AC.reference(name)
    zero = np.flatnonzero(res.trace[0, :res.rounds, 0] == 0)
    assert zero.size and int(zero[0]) < rounds // 2                               # (c)
    assert int(zero[0]) == AC.FIRST_ZERO[name]           # what the cases' docstring says
    assert res.nfail[0] == 0 == res.cost[0] and res.winner == 0 and res.rounds % 8 == 0
    assert AC.values_fn(name)(np.asarray(res.leaves[0])[:, :, None])[0].all()


def test_walk_ref_without_aims_is_unchanged():
    """aims=None is today's loop (the references of tests/tree_cases.py are
    computed without the argument); an empty table gives the same walk."""
    name = "conj"
    prog, T = TC.program(name), TC.trees(name)
    want = TC.reference(name, 2, 256, 8)
    got = RP.walk_ref(TC.values_fn(name), default_leafgen(prog), TC.consts_of(prog),
                      TC.starts(name, 2), T.roots, TC.SEED, 256, 8, 8, score=RP.tree_scoring(T),
                      aims=RP.no_aims())
    for a, b in ((got.leaves, want.leaves), (got.nfail, want.nfail), (got.cost, want.cost),
                 (got.trace, want.trace)):
        assert np.array_equal(a, b)
    assert got.rounds == want.rounds and got.winner == want.winner


# ---------------------------------------------------------------------------
# the resolution rules
# ---------------------------------------------------------------------------

def rule_rows():
    """(name, destination term, the other side, pieces, exact): ``exact``: no
    ite guard and no numeral part, so applying the entry makes the equality
    hold.  Every row has symbols of its own; the other side never resolves."""
    rows = []

    def other(tag, w):
        return N.bv_op("bvmul", N.bv_var("m_" + tag, w), N.bv_var("n_" + tag, w))

    def row(tag, dest, pieces, exact):
        rows.append((tag, dest, other(tag, dest.width), pieces, exact))
    v = lambda s, w: N.bv_var(s, w)
    row("var", v("va", 16), 1, True)
    row("concat", N.concat(v("ca", 8), v("cb", 8)), 2, True)
    row("concat_num", N.concat(v("na", 8), N.bv_num(5, 4), v("nb", 4)), 2, False)
    row("extract", N.extract(11, 4, v("ea", 16)), 1, True)
    row("extract_concat", N.extract(11, 4, N.concat(v("xa", 8), v("xb", 8))), 2, True)
    row("extract_miss", N.extract(7, 2, N.concat(v("ma", 8), v("mb", 8))), 1, True)
    row("zext", N.zero_extend(8, v("za", 8)), 1, False)
    guard = N.bv_cmp("bvult", v("ga", 8), v("gb", 8))
    # (an ite that is a whole side is a case split of distance_trees: its
    # arms become atoms of their own; below a concat it is a destination)
    row("ite_then", N.concat(N.ite(guard, v("ia", 8), N.bv_num(7, 8)), v("ib", 8)), 2, False)
    row("ite_else", N.concat(v("jb", 8), N.ite(guard, N.bv_num(7, 8), v("ja", 8))), 2, False)
    row("select", N.select(N.array_var("A", 8, 8), N.bv_num(3, 8)), 1, True)
    row("select2", N.concat(N.select(N.array_var("A", 8, 8), N.bv_num(200, 8)), v("sa", 8)), 2, True)
    row("wide_var", N.extract(279, 250, v("wv", 300)), 2, True)
    return rows


@pytest.fixture(scope="module")
def rules():
    with N.fresh_scope():
        rows = rule_rows()
        cs = [N.eq(dest, oth) for _, dest, oth, _, _ in rows]
        both = N.eq(N.bv_var("ba", 16), N.bv_var("bb", 16))          # both sides resolve
        cs.append(both)
        T = RP.distance_trees(cs)
        prog = compile_constraints(cs, CS.mask_probes(cs) + CS.mask_probes(T.atom_nodes)
                                   + list(T.probes), const_keys=True)
    return rows, cs, T, prog, RP.aim_table(T, prog)


def test_rules_give_the_expected_entries(rules):
    rows, cs, T, prog, A = rules
    assert T.n_resid == len(cs) and not any(T.is_tree(k) for k in range(len(cs)))
    assert prog.table_ckeys["A"] == [3, 200] or sorted(prog.table_ckeys["A"]) == [3, 200]
    # one entry per row (side a), two for the last (a, then b)
    assert [int(e[0]) for e in A.entries] == list(range(len(rows))) + [len(rows)] * 2
    assert A.sides == [0] * len(rows) + [0, 1]
    assert [int(e[2]) for e in A.entries[:len(rows)]] == [r[3] for r in rows]
    by = {r[0]: A.of(i) for i, r in enumerate(rows)}
    name = lambda p: prog.leaves[p[0]].name
    assert by["extract"] == [(prog.leaf_index()[name(by["extract"][0])], 4, 0, 8)]
    assert [p[1:] for p in by["extract_concat"]] == [(0, 4, 4), (4, 0, 4)]
    assert [p[1:] for p in by["extract_miss"]] == [(2, 0, 6)]         # mb alone, clipped
    assert [p[1:] for p in by["concat_num"]] == [(0, 8, 8), (0, 0, 4)]
    assert [p[1:] for p in by["wide_var"]] == [(250, 0, 6), (0, 6, 24)]
    assert [prog.leaves[p[0]].chunk for p in by["wide_var"]] == [0, 1]
    assert prog.leaves[by["select"][0][0]].kind == "cval"
    assert prog.table_ckeys["A"][prog.leaves[by["select"][0][0]].entry] == 3
    assert prog.table_ckeys["A"][prog.leaves[by["select2"][0][0]].entry] == 200
    for e in range(len(A)):
        for leaf, leaf_bit, value_bit, n in A.of(e):
            assert n >= 1 and leaf_bit + n <= prog.leaves[leaf].width and value_bit + n <= 256


def _assignment(prog, rng):
    vars_, table = {}, [(int(k), int(rng.integers(256))) for k in (3, 200)]
    for l in prog.leaves:
        if l.kind == "var" and l.source not in vars_:
            w = 300 if l.source == "wv" else l.width
            vars_[l.source] = int.from_bytes(rng.bytes(40), "little") & ((1 << w) - 1)
    return R.Assignment(vars_, {"A": (table, 0)}, {})


def _rows_of(prog, asg):
    out = np.zeros((len(prog.leaves), 8), dtype=np.uint32)
    for i, l in enumerate(prog.leaves):
        if l.kind == "var":
            v = asg.vars[l.source] >> (256 * l.chunk) & ((1 << l.width) - 1)
        else:
            assert l.kind == "cval" and l.source == "A"
            v = dict(asg.arrays["A"][0])[prog.table_ckeys["A"][l.entry]]
        out[i] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    return out


def _asg_of(prog, rows):
    vals = RP._ints(rows)
    vars_, table = {}, []
    for i, l in enumerate(prog.leaves):
        if l.kind == "var":
            vars_[l.source] = vars_.get(l.source, 0) | vals[i] << (256 * l.chunk)
        else:
            table.append((prog.table_ckeys["A"][l.entry], vals[i]))
    return R.Assignment(vars_, {"A": (table, 0)}, {})


@pytest.mark.parametrize("seed", range(3))
def test_every_rule_against_the_oracle(rules, seed):
    """One entry applied (by the library, lane 1 of 8) to a random assignment:
    only the named bits change, they change by the residual's bits, and an
    exact shape's equality then holds in the oracle."""
    rows, cs, T, prog, A = rules
    rng = np.random.default_rng(seed)
    gens, consts = default_leafgen(prog), AC.consts_of(prog)
    exact = [r[4] for r in rows] + [True, True]
    for _ in range(4):
        asg = _assignment(prog, rng)
        base = _rows_of(prog, asg)
        resid = R.evaluate(T.probes, asg)
        rvals = np.array([np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u4")
                          for v in resid], dtype=np.uint32)
        for e in range(len(A)):
            p = int(A.entries[e, 0])
            one = RP.make_aims([(p, A.of(e))])
            out, moves = walk_aim_mutate_host(gens, consts, base, rvals, one, 1, 0, 8)
            assert np.array_equal(out, RP.aim_mutate_ref(gens, consts, base, rvals, one, 1, 0, 8))
            if resid[p] == 0:
                assert moves[1, 4] == NONE
                continue
            assert moves[1].tolist() == [0, moves[1, 1], moves[1, 2], moves[1, 3], 0]
            new, old = RP._ints(out[:, :, 1]), RP._ints(base)
            want = {}
            for leaf, leaf_bit, value_bit, n in A.of(e):
                want[leaf] = want.get(leaf, 0) | (resid[p] >> value_bit & ((1 << n) - 1)) << leaf_bit
            for i in range(len(old)):
                assert new[i] ^ old[i] == want.get(i, 0), (rows[min(e, len(rows) - 1)][0], i)
            after = R.evaluate([cs[p]], _asg_of(prog, out[:, :, 1]))[0]
            if exact[e]:
                assert after, rows[min(e, len(rows) - 1)][0]


def test_what_does_not_resolve_and_what_is_dropped():
    with N.fresh_scope():
        v = lambda s, w: N.bv_var(s, w)
        A2, i8 = N.array_var("B", 8, 8), v("i", 8)
        t = lambda tag, w: N.bv_op("bvmul", v("m" + tag, w), v("n" + tag, w))
        bits65 = N.concat(*[v("o%02d" % k, 1) for k in range(65)])
        cs = [N.eq(N.bv_op("bvadd", v("a", 8), v("b", 8)), t("0", 8)),            # arithmetic
              N.eq(N.concat(v("c", 8), N.bv_op("bvadd", v("d", 8), v("e", 8))), t("1", 16)),
              N.eq(N.select(A2, i8), t("2", 8)),                                   # symbolic key
              N.eq(N.concat(N.ite(N.bv_cmp("bvult", v("f", 8), v("g", 8)), v("h", 8), v("k", 8)),
                            v("q", 8)), t("3", 16)),                               # no numeral arm
              N.eq(N.bv_op("bvnot", v("l", 8)), t("4", 8)),
              N.eq(bits65, t("5", 65)),                                            # 65 pieces
              N.eq(N.select(A2, N.bv_num(9, 8)), t("6", 8)),                       # this one resolves
              N.eq(N.sign_extend(8, v("p", 8)), t("7", 16))]
        T = RP.distance_trees(cs)
        prog = compile_constraints(cs, CS.mask_probes(cs) + CS.mask_probes(T.atom_nodes)
                                   + list(T.probes), const_keys=True)
    A = RP.aim_table(T, prog)
    assert len(A) == 1 and prog.leaves[A.of(0)[0][0]].kind == "cval"
    assert RP.aim_pieces(cs[3].args[0], prog) is None
    assert len(RP.aim_pieces(bits65, prog)) == 65
    # a key that the presets fold to a constant the program reads
    folded = dataclasses.replace(prog, presets=types.SimpleNamespace(subst={i8.id: 9}))
    assert RP.aim_pieces(N.select(A2, i8), prog) is None
    assert RP.aim_pieces(N.select(A2, i8), folded) == A.of(0)
    off = dataclasses.replace(prog, presets=types.SimpleNamespace(subst={i8.id: 10}))
    assert RP.aim_pieces(N.select(A2, i8), off) is None
    # a leaf the construction derives: moving it does nothing
    derived = dataclasses.replace(prog, derived={A.of(0)[0][0]: 0})
    assert len(RP.aim_table(T, derived)) == 0


def test_at_most_256_entries_the_first_ones():
    with N.fresh_scope():
        cs = [N.eq(N.bv_var("x%03d" % k, 8), N.bv_var("y%03d" % k, 8)) for k in range(130)]
        T = RP.distance_trees(cs)
        prog = compile_constraints(cs, CS.mask_probes(cs) + list(T.probes))
    A = RP.aim_table(T, prog)
    assert len(A) == 256 and [int(e[0]) for e in A.entries] == [k // 2 for k in range(256)]
    assert A.sides == [0, 1] * 128


# ---------------------------------------------------------------------------
# the lane function: the library against the specification
# ---------------------------------------------------------------------------

WIDTHS = (256, 100, 13, 143, 8, 64, 33)
N_RESID = 48


def synthetic(seed, n_entries):
    """(leafgen, consts, base, rvals, aims): seven leaves, entry 0 of one
    piece, entry 1 of 64, the others of 1 .. 6 pieces anywhere inside their
    leaves and the residual; a third of the residuals zero."""
    rng = np.random.default_rng(seed)
    consts = rng.integers(0, 1 << 32, size=(6, 8), dtype=np.uint64).astype(np.uint32)
    gens = [LeafGen(w, 2 * (i % 2), 3 * (i % 2), 50, 70, 85) for i, w in enumerate(WIDTHS)]
    base = rng.integers(0, 1 << 32, size=(len(WIDTHS), 8), dtype=np.uint64).astype(np.uint32)
    for i, w in enumerate(WIDTHS):
        v = RP._ints(base[i:i + 1])[0] & ((1 << w) - 1)
        base[i] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    rvals = rng.integers(0, 1 << 32, size=(N_RESID, 8), dtype=np.uint64).astype(np.uint32)
    rvals[rng.integers(0, 3, size=N_RESID) == 0] = 0
    rvals[:2] |= 1                                       # entries 0 and 1 are live

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
        entries.append((e % N_RESID, ps))
    return gens, consts, base, rvals, RP.make_aims(entries)


@pytest.mark.parametrize("lanes", [1, 7, 8, 63, 64, 65, 256, 4096])
@pytest.mark.parametrize("n_entries", [0, 1, 5, 40])
def test_library_lanes_equal_the_specification(lanes, n_entries):
    gens, consts, base, rvals, A = synthetic(lanes * 64 + n_entries, n_entries)
    live = [e for e in range(n_entries) if rvals[e % N_RESID].any()]
    cap = lanes // 8
    n1 = min(len(live), cap)
    landed = 0
    for r, rv in ((0, None), (0, rvals), (3, rvals), (65535, rvals)):
        want = RP.aim_mutate_ref(gens, consts, base, rv, A, 0xA11CE, r, lanes)
        got, moves = walk_aim_mutate_host(gens, consts, base, rv, A, 0xA11CE, r, lanes,
                                          n_resid=N_RESID)
        assert np.array_equal(got, want)
        picks = RP.aim_picks_ref(rv, A, r, lanes)
        assert np.array_equal(moves[:, 4].astype(np.int64), picks)
        plain, pmoves = repair_mutate_host(gens, consts, base, 0xA11CE, r, lanes)
        if rv is None:                                   # round 0: today's neighbours
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
                if leaf in {p[0] for p in A.of(int(picks[j]))} and \
                        (m + 1 == int(moves[j, 0]) or int(moves[j, 3]) != leaf):
                    landed += 1
                    assert np.array_equal(got[leaf, :, j], plain[leaf, :, j])
    if n_entries >= 5 and lanes >= 64:
        assert landed > 0
    if n_entries == 40 and 8 <= lanes <= 65:
        assert len(live) > cap                           # above the cap: the list rotates
    if n_entries == 5 and lanes >= 64:
        assert 0 < len(live) <= cap


def test_lane_ranges_of_the_host_entry():
    gens, consts, base, rvals, A = synthetic(7, 12)
    whole, moves = walk_aim_mutate_host(gens, consts, base, rvals, A, 9, 2, 300, n_resid=N_RESID)
    part, pm = walk_aim_mutate_host(gens, consts, base, rvals, A, 9, 2, 300, lane0=5, n_lanes=60,
                                    n_resid=N_RESID)
    assert np.array_equal(part, whole[:, :, 5:65]) and np.array_equal(pm, moves[5:65])


@pytest.mark.parametrize("lanes", [1, 64, 1000])
def test_an_empty_table_is_the_plain_move_function(lanes):
    gens, consts, base, rvals, _ = synthetic(3, 0)
    for r in (0, 9):
        want, wm = repair_mutate_host(gens, consts, base, 77, r, lanes)
        got, gm = walk_aim_mutate_host(gens, consts, base, rvals, RP.no_aims(), 77, r, lanes,
                                       n_resid=N_RESID)
        assert np.array_equal(got, want) and np.array_equal(gm[:, :4], wm)
        assert (gm[:, 4] == NONE).all()


MALFORMED = {
    "residual index at n_resid": [(N_RESID, [(0, 0, 0, 8)])],
    "an entry without pieces": [(0, [])],
    "65 pieces": [(0, [(4, 0, 0, 1)] * 65)],
    "leaf at n_leaves": [(0, [(len(WIDTHS), 0, 0, 1)])],
    "leaf_bit + len above the width": [(0, [(2, 6, 0, 8)])],
    "leaf_bit above the width": [(0, [(2, 14, 0, 1)])],
    "value_bit + len above 256": [(0, [(0, 0, 250, 7)])],
    "value_bit above 256": [(0, [(0, 0, 300, 1)])],
    "len 0": [(0, [(0, 0, 0, 0)])],
    "len above 256": [(0, [(0, 0, 0, 257)])],
    "257 entries": [(0, [(0, 0, 0, 1)])] * 257,
}


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_malformed_tables_are_refused(kind):
    gens, consts, base, rvals, _ = synthetic(1, 0)
    with pytest.raises(EngineError):
        walk_aim_mutate_host(gens, consts, base, rvals, RP.make_aims(MALFORMED[kind]), 1, 1, 64,
                             n_resid=N_RESID)


def test_pieces_outside_the_piece_array_are_refused():
    gens, consts, base, rvals, _ = synthetic(1, 0)
    ok = RP.make_aims([(0, [(0, 0, 0, 8), (1, 0, 8, 8)])])
    walk_aim_mutate_host(gens, consts, base, rvals, ok, 1, 1, 64, n_resid=N_RESID)
    for off, cnt in ((1, 2), (2, 1), (3, 1), (0xFFFFFFFF, 2), (0, 3)):
        bad = RP.Aims(np.array([[0, off, cnt]], dtype=np.uint32), ok.pieces, [0])
        with pytest.raises(EngineError):
            walk_aim_mutate_host(gens, consts, base, rvals, bad, 1, 1, 64, n_resid=N_RESID)

"""The walk with aims through sums, differences, masks and shifts (DESIGN.md
§3.15) without a GPU: the mask and shift rules of the side resolver against a
brute force over the oracle, linear sides and their eligibility, the caps of
sum_probes and sum_table, the library's lane function (mg_walk_sum_mutate_host)
against the specification (repair.sum_mutate_ref), the validator, and the
crafted cases of tests/sum_cases.py."""

import hashlib

import numpy as np
import pytest

import aim_cases as AC
import sum_cases as SC
import uf_cases as UC
import walk_cases as WK
from mythril_amd import repair as RP
from mythril_amd.engine import (EngineError, LeafGen, default_leafgen, walk_sum_mutate_host,
                                walk_uf_mutate_host)
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N
from oracle import smtlib_ref as R

NONE = RP.AIM_NONE
XOR, LOW, LOW_S, HIGH, HIGH_S = range(5)


# ---------------------------------------------------------------------------
# the crafted cases
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", SC.STUCK)
def test_crafted_cases_need_the_sum_aims(name):
    """The conditions on the inputs, none of them a measurement: (a) the
    generator finds no model among lanes x max_rounds candidates, (b) walk_ref
    with the tree scoring and the tables of §3.14 is still failing after
    max_rounds from the same start, (c) with the tables of §3.15 it reaches a
    model within half of max_rounds."""
    rounds = SC.MAX_ROUNDS[name]
    B, U, S = SC.tables(name)
    prog = SC.program(name)
    leaf = {l.source: i for i, l in enumerate(prog.leaves)}
    modes, lin = [int(m) for m in B.entries[:, 3]], [int(w) for w in S.lin]
    if name == "sum":
        # a + b: both terms, +, one side row; p xor q resolves by no rule
        assert modes == [XOR, XOR] and lin == [RP.SUM_LINEAR] * 2 and S.n_srows == 1
        assert [B.of(e) for e in (0, 1)] == [[(leaf["a"], 0, 0, 256)], [(leaf["b"], 0, 0, 256)]]
        assert len(SC.old_tables(name)[0]) == 0
    elif name == "spend":
        neg = RP.SUM_LINEAR | RP.SUM_NEG
        assert modes == [XOR] * 20 + [HIGH_S, HIGH_S, LOW, LOW] and S.n_srows == 0
        assert lin == [0] * 20 + [RP.SUM_LINEAR, neg, RP.SUM_LINEAR, neg]
        assert B.of(20) == B.of(22) == [(leaf["bal"], 0, 128, 128), (leaf["bal"], 128, 0, 128)]
        assert B.of(21) == B.of(23) == [(leaf["v"], 0, 0, 256)]
        assert [int(t) for t in B.entries[20:, 4]] == [0, 0, 1, 1]
        assert len(SC.old_tables(name)[0]) == 20 and SC.old_tables(name)[0].n_order == 0
    else:
        # y * z resolves by no rule and need not: the one target is x, negative
        assert modes == [XOR] and lin == [RP.SUM_LINEAR | RP.SUM_NEG] and S.n_srows == 1
        assert B.of(0) == [(leaf["x"], 0, 0, 256)]
        assert len(SC.old_tables(name)[0]) == 0
    assert len(U) == 0
    start = SC.start_rows(name)
    assert (~SC.values_fn(name)(start[:, :, None])[0][0]).sum() == 1
    assert SC.generator_hits(name, SC.LANES * rounds) == 0                        # (a)
    stuck = SC.reference(name, sums=False)
    assert stuck.nfail[0] > 0 and stuck.rounds == rounds                          # (b)
    res = SC.reference(name)
    zero = SC.first_zero(res)
    assert zero is not None and zero < rounds // 2                                # (c)
    assert zero == SC.FIRST_ZERO[name]                   # what the cases' docstring says
    assert res.nfail[0] == 0 == res.cost[0] and res.winner == 0 and res.rounds % 8 == 0
    assert SC.values_fn(name)(np.asarray(res.leaves[0])[:, :, None])[0].all()


def test_selector_closes_in_round_one_by_the_mask_and_shift_rules_alone():
    B, U, S = SC.tables("selector")
    assert S.n_linear == 0 and S.n_srows == 0 and len(U) == 0
    assert [int(m) for m in B.entries[:, 3]] == [XOR] and B.of(0) == [(0, 224, 0, 32)]
    assert len(SC.old_tables("selector")[0]) == 0
    assert SC.generator_hits("selector", SC.LANES * SC.MAX_ROUNDS["selector"]) == 0
    new, old = SC.reference("selector"), SC.reference("selector", sums=False)
    assert SC.first_zero(new) == 1 == SC.FIRST_ZERO["selector"]
    late = SC.first_zero(old)
    assert late is None or late > 1
    assert late == SC.SELECTOR_OLD                       # what the cases' docstring says
    assert SC.values_fn("selector")(np.asarray(new.leaves[0])[:, :, None])[0].all()


def test_without_a_linear_entry_walk_ref_is_the_walk_of_uf():
    """`hash` of tests/uf_cases.py through sums=: the same walk, bit for bit."""
    name = "hash"
    prog, T = UC.program(name), UC.trees(name)
    B, U = UC.tables(name)
    B2, U2, S = RP.sum_table(UC.case(name)[0], T, prog, UC.apps(name))
    assert S.n_linear == 0 and S.n_srows == 0
    for a, b in ((B.entries, B2.entries), (B.pieces, B2.pieces), (B.fixed, B2.fixed),
                 (U.slots, U2.slots), (U.cands, U2.cands)):
        assert np.array_equal(a, b)
    want = UC.reference(name, 2, 256, 8)
    fn = UC.values_fn(name)
    with_rows = lambda soa: fn(soa) + (np.zeros((0, 8, soa.shape[2]), dtype=np.uint32),)
    got = RP.walk_ref(with_rows, default_leafgen(prog), UC.consts_of(prog), UC.starts(name, 2),
                      T.roots, UC.SEED, 256, 8, 8, score=RP.tree_scoring(T), bounds=B2, ufs=U2,
                      sums=S)
    for a, b in ((got.leaves, want.leaves), (got.nfail, want.nfail), (got.cost, want.cost),
                 (got.trace, want.trace)):
        assert np.array_equal(a, b)
    assert got.rounds == want.rounds and got.winner == want.winner


# ---------------------------------------------------------------------------
# the mask and shift rules of the side resolver
# ---------------------------------------------------------------------------

W = 16


def _resolved(term):
    """(program, pieces, fixed) of a 16-bit term over the variables x and y."""
    prog = compile_constraints([N.eq(term, N.bv_num(0x1234, term.width))], [], nreg=16)
    side = RP._resolve_side(term, prog, None, True)
    return (prog,) + (side if side is not None else (None, None))


def _brute(term, rng, n=64):
    """Scatter values through the pieces and evaluate the term with the
    oracle: every bit of the term is the scattered bit, or its fixed bit."""
    prog, pieces, fixed = _resolved(term)
    assert pieces is not None
    covered = 0
    for _, _, vb, ln in pieces:
        assert covered & (((1 << ln) - 1) << vb) == 0    # no two pieces write one bit
        covered |= ((1 << ln) - 1) << vb
    assert covered & fixed == 0
    for _ in range(n):
        val = int(rng.integers(0, 1 << term.width))
        leaves = [int(rng.integers(0, 1 << l.width)) for l in prog.leaves]
        for l, lb, vb, ln in pieces:
            m = (1 << ln) - 1
            leaves[l] = leaves[l] & ~(m << lb) | (val >> vb & m) << lb
        asg = R.Assignment({l.source: leaves[i] for i, l in enumerate(prog.leaves)})
        assert R.evaluate([term], asg)[0] == fixed | val & covered
    return pieces, fixed


def _xy():
    return N.bv_var("x", W), N.bv_var("y", W)


@pytest.mark.parametrize("mask", [0x8001, 0x0100, 0xFFFF, 0x0000, 0x3C3C, 0xF00F, 0x7FFE])
@pytest.mark.parametrize("op", ["bvand", "bvor"])
def test_masks_cut_the_pieces_to_their_runs(op, mask):
    """Runs at both ends, a single-bit run, all ones and zero; either operand
    order; under a concat with a numeral, so that fixed bits pass through."""
    rng = np.random.default_rng(mask + len(op))
    x, y = _xy()
    inner = N.concat(N.extract(7, 0, x), N.bv_num(0x5, 4), N.extract(3, 0, y))
    for term in (N.bv_op(op, inner, N.bv_num(mask, W)), N.bv_op(op, N.bv_num(mask, W), inner)):
        pieces, fixed = _brute(term, rng)
        keep = mask if op == "bvand" else ~mask & 0xFFFF
        assert sum(ln for *_, ln in pieces) == bin(keep & 0xFF0F).count("1")
        assert fixed == ((0x0050 & mask) if op == "bvand" else (0x0050 & ~mask | mask))
    # n-ary with exactly one non-numeral operand
    term = N.bv_op(op, N.bv_num(mask, W), x, N.bv_num(0x0FF0, W))
    _brute(term, rng)
    assert _resolved(N.bv_op(op, x, y, N.bv_num(mask, W)))[1] is None
    assert _resolved(N.bv_op(op, x, y))[1] is None


@pytest.mark.parametrize("c", [0, 1, 5, W - 1])
def test_shifts_by_a_numeral_are_extracts_and_concats(c):
    rng = np.random.default_rng(c)
    x, y = _xy()
    inner = N.concat(N.extract(7, 0, x), N.bv_num(0x9, 4), N.extract(3, 0, y))
    k = N.bv_num(c, W)
    right = [N.bv_op("bvlshr", inner, k), N.bv_op("bvudiv", inner, N.bv_num(1 << c, W))]
    left = [N.bv_op("bvshl", inner, k), N.bv_op("bvmul", inner, N.bv_num(1 << c, W)),
            N.bv_op("bvmul", N.bv_num(1, W), inner, N.bv_num(1 << c, W))]
    want_r = _brute(N.zero_extend(c, N.extract(W - 1, c, inner)), rng) if c else \
        _brute(inner, rng)
    for term in right:
        assert _brute(term, rng) == want_r
    want_l = _brute(N.concat(N.extract(W - 1 - c, 0, inner), N.bv_num(0, c)), rng) if c else \
        _brute(inner, rng)
    for term in left:
        assert _brute(term, rng) == want_l
    # not a power of two, a symbolic amount, two non-numeral factors
    for term in (N.bv_op("bvudiv", x, N.bv_num(6, W)), N.bv_op("bvmul", x, N.bv_num(6, W)),
                 N.bv_op("bvlshr", x, y), N.bv_op("bvshl", x, y), N.bv_op("bvmul", x, y),
                 N.bv_op("bvudiv", N.bv_num(1 << c, W), x)):
        assert _resolved(term)[1] is None


def test_the_selector_word_resolves_and_the_rules_are_off_by_default():
    w = N.bv_var("w", 256)
    word = N.bv_op("bvand", N.bv_num(0xffffffff, 256), N.bv_op("bvudiv", w, N.bv_num(1 << 224, 256)))
    prog = compile_constraints([N.eq(word, N.bv_num(SC.SELECTOR, 256))], [], nreg=16)
    assert RP._resolve_side(word, prog, None, True) == ([(0, 224, 0, 32)], 0)
    assert RP.aim_pieces(word, prog, None, True) == [(0, 224, 0, 32)]
    assert RP._resolve_side(word, prog) is None and RP.aim_pieces(word, prog) is None
    assert RP.aim_refusal(word, prog) == "bvand is not a destination"
    assert RP.aim_refusal(word, prog, None, True) is None
    x = N.bv_var("x", 256)
    odd = N.bv_op("bvand", N.bv_num(0xff, 256), N.bv_op("bvudiv", w, x))
    prog = compile_constraints([N.eq(odd, N.bv_num(1, 256))], [], nreg=16)
    assert RP.aim_refusal(odd, prog, None, True) == "bvudiv: not one operand and a numeral 2^c"
    assert RP.aim_refusal(N.bv_op("bvand", w, x), prog, None, True) == \
        "bvand: not one operand and numerals"


# what aim_table, bound_table and uf_table give on every case of the earlier
# walks, recorded before the rules were added: sha256 over their arrays
TABLES = {"aim_cases.bytes": "0e0cc88da355a6d4", "aim_cases.odd": "12f63e0bc43cb2e4",
          "aim_cases.wide": "ade0f103d61153e9", "uf_cases.ckey": "a2a561603b5afa9a",
          "uf_cases.hash": "626df0148f3056f6", "uf_cases.rekey": "5f66ecb4f33b6eec",
          "uf_cases.shadow": "00918086e56f74ee", "walk_cases.hamming": "46b027eba3e1a294",
          "walk_cases.magnitude": "dcc86096e9804ddc", "walk_cases.mixed": "38138b251b2a5444"}


@pytest.mark.parametrize("key", sorted(TABLES))
def test_with_the_rules_off_every_earlier_table_is_unchanged(key):
    mod, name = key.split(".")
    C = {"aim_cases": AC, "walk_cases": WK, "uf_cases": UC}[mod]
    cs, prog = C.case(name)[0], C.program(name)
    T = C.trees(name) if hasattr(C, "trees") else RP.distance_trees(cs)
    apps = list(C.apps(name)) if hasattr(C, "apps") else []
    A, B = RP.aim_table(T, prog), RP.bound_table(cs, T, prog)
    B2, U = RP.uf_table(cs, T, prog, apps)
    h = hashlib.sha256()
    for a in (A.entries, A.pieces, B.entries, B.pieces, B.fixed, B2.entries, B2.pieces, B2.fixed,
              U.slots, U.funcs, U.cands, U.ukeys):
        h.update(np.ascontiguousarray(a, dtype=np.uint32).tobytes())
        h.update(b"|")
    assert h.hexdigest()[:16] == TABLES[key]


# ---------------------------------------------------------------------------
# linear sides
# ---------------------------------------------------------------------------

def _v(names, w=64):
    return [N.bv_var(s, w) for s in names]


def _signs(t):
    terms = RP.linear_terms(t)
    return None if terms is None else [(s, x.params[0] if x.op == "var" else x.op) for s, x in terms]


def test_flattening_takes_sums_differences_and_negations_at_the_top_only():
    a, b, c, d, e = _v("abcde")
    op, num = N.bv_op, lambda v: N.bv_num(v, 64)
    assert _signs(op("bvsub", a, op("bvsub", b, c))) == [(1, "a"), (-1, "b"), (1, "c")]
    assert _signs(op("bvadd", op("bvneg", op("bvadd", a, num(3))), b)) == [(-1, "a"), (1, "b")]
    assert _signs(op("bvadd", a, b, c, d)) == [(1, "a"), (1, "b"), (1, "c"), (1, "d")]
    assert _signs(op("bvadd", a, op("bvadd", b, op("bvadd", c, num(1))))) == \
        [(1, "a"), (1, "b"), (1, "c")]
    assert _signs(op("bvadd", a, num(3))) == [(1, "a")]
    assert _signs(op("bvneg", a)) == [(-1, "a")]
    assert _signs(op("bvsub", op("bvmul", a, b), c)) == [(1, "bvmul"), (-1, "c")]
    # a single positive term with no numeral is the plain rule; five terms; a
    # numeral alone; wider than 256 bits; a sum under an extract
    assert _signs(a) is None and _signs(op("bvadd", a, b, c, d, e)) is None
    assert _signs(op("bvadd", num(1), num(2))) is None
    wide = _v("xy", 257)
    assert RP.linear_terms(op("bvadd", *wide)) is None
    assert RP.linear_terms(N.extract(31, 0, op("bvadd", a, b))) is None


def _program(cs, **kw):
    return compile_constraints(cs, [], nreg=16, **kw)


def test_eligibility_refuses_shared_and_unresolved_terms():
    a, b, c = _v("abc")
    op, num = N.bv_op, lambda v: N.bv_num(v, 64)
    f = lambda x: N.apply_uf("f", 64, 64, x)
    side = op("bvadd", a, op("bvmul", a, b), c)
    prog = _program([N.eq(side, num(7))])
    leaf = {l.source: i for i, l in enumerate(prog.leaves) if l.kind == "var"}
    assert RP.sum_target(side, 0, prog) == "a leaf shared with another term"
    assert RP.sum_target(side, 1, prog) == "bvmul: not one operand and a numeral 2^c"
    assert RP.sum_target(side, 2, prog) == (1, [(leaf["c"], 0, 0, 64)], 0)
    # x - x; a target under a mask, with numeral bits; a term that is a UF
    # application stands in no one's way
    side = op("bvsub", a, a)
    assert RP.sum_target(side, 0, _program([N.eq(op("bvadd", side, b), num(7))])) == \
        "a leaf shared with another term"
    side = op("bvsub", f(b), op("bvor", a, num(0xF0)))
    prog = _program([N.eq(side, num(7))])
    la = next(i for i, l in enumerate(prog.leaves) if l.kind == "var" and l.source == "a")
    assert RP.sum_target(side, 1, prog) == (-1, [(la, 0, 0, 4), (la, 8, 8, 56)], 0xF0)
    assert isinstance(RP.sum_target(side, 0, prog), str)
    assert RP.aim_refusal(side, prog, None, True) is None
    both = op("bvadd", op("bvmul", a, b), op("bvmul", b, c))
    assert RP.aim_refusal(both, _program([N.eq(both, num(1))]), None, True) == \
        "bvadd: no eligible target (bvmul: not one operand and a numeral 2^c)"


def test_a_derived_leaf_is_no_target():
    """Solve form: x is defined by the equality x = y + 1, so only y moves."""
    from mythril_amd.model import _compile_search_uncached
    x, y, z = _v("xyz", 256)
    op, num = N.bv_op, lambda v: N.bv_num(v, 256)
    side = op("bvadd", x, z)
    cs = [N.eq(x, op("bvmul", y, y)), N.bv_cmp("bvult", side, num(100))]
    T = RP.distance_trees(cs)
    prog = _compile_search_uncached(cs, tuple(T.probes))
    lx = next(i for i, l in enumerate(prog.leaves) if l.kind == "var" and l.source == "x")
    lz = next(i for i, l in enumerate(prog.leaves) if l.kind == "var" and l.source == "z")
    assert lx in prog.derived and lz not in prog.derived
    assert RP.sum_target(side, 0, prog) == "a term on a derived leaf"
    assert RP.sum_target(side, 1, prog) == (1, [(lz, 0, 0, 256)], 0)
    B, U, S = RP.sum_table(cs, T, prog, [])
    assert [B.of(e) for e in range(len(B)) if S.lin[e]] == [[(lz, 0, 0, 256)]]


def _many(n, rhs_var=False):
    cs = []
    for i in range(n):
        a, b = _v(["a%03d" % i, "b%03d" % i], 16)
        cs.append(N.eq(N.bv_op("bvadd", a, b),
                       N.bv_var("c%03d" % i, 16) if rhs_var else N.bv_num(i + 1, 16)))
    return cs


def test_sixty_five_linear_sides_are_cut_to_sixty_four_rows():
    cs = _many(65)
    T = RP.distance_trees(cs)
    rows = RP.sum_probes(T)
    assert len(rows) == RP.SUM_MAX_ROWS and [t.id for t in rows] == [c.args[0].id for c in cs[:64]]
    prog = compile_constraints(cs, list(T.probes) + rows, nreg=16)
    B, U, S = RP.sum_table(cs, T, prog, [])
    # the side past the rows gets no XOR entry
    assert len(B) == 128 and S.n_srows == 64 and S.n_linear == 128
    assert sorted(set(int(w) >> RP.SUM_ROW_SHIFT for w in S.lin)) == list(range(64))
    assert [int(p) for p in B.entries[:, 0]] == [i // 2 for i in range(128)]
    # one row per distinct side: a side read twice has one
    twice = cs[:2] + [N.eq(cs[0].args[0], N.bv_num(9, 16))]
    assert len(RP.sum_probes(RP.distance_trees(twice))) == 2


def test_the_table_is_cut_to_256_entries():
    cs = _many(64, rhs_var=True) + [N.bv_cmp("bvult", N.bv_op("bvadd", *_v(["p%d" % i, "q%d" % i], 16)),
                                             N.bv_var("r%d" % i, 16)) for i in range(40)]
    T = RP.distance_trees(cs)
    prog = compile_constraints(cs, list(T.probes) + RP.sum_probes(T), nreg=16)
    B, U, S = RP.sum_table(cs, T, prog, [])
    # 64 x (a, b linear, c plain) = 192 XOR entries, then 40 x (p, q LOW_STRICT
    # linear, r HIGH_STRICT plain) = 120 order entries: the first 64 of them
    assert len(B) == RP.AIM_MAX_ENTRIES == len(S.lin)
    assert int((B.entries[:, 3] == XOR).sum()) == 192 and S.n_linear == 128 + 43
    assert [int(w) for w in S.lin[:3]] == [RP.SUM_LINEAR, RP.SUM_LINEAR | 0, 0]
    assert [int(m) for m in B.entries[192:195, 3]] == [LOW_S, LOW_S, HIGH_S]
    assert [int(w) for w in S.lin[192:195]] == [RP.SUM_LINEAR, RP.SUM_LINEAR, 0]


# ---------------------------------------------------------------------------
# the library's lane function against the specification
# ---------------------------------------------------------------------------

def _row(v):
    return np.frombuffer((int(v) & RP.M256).to_bytes(32, "little"), dtype="<u4")


def _rand(rng, bits=256):
    return int.from_bytes(rng.bytes(32), "little") >> (256 - bits)


def synthetic(rng, random_table=False):
    """Six 256-bit leaves and two 64-bit ones, three residuals, two side rows;
    every mode with both signs, a target with numeral bits, a target of two
    pieces, entries that are not linear between them."""
    gens = [LeafGen(256, 0, 0, 0, 0, 0) for _ in range(6)] + [LeafGen(64, 0, 0, 0, 0, 0)] * 2
    base = np.stack([_row(_rand(rng, 256 if i < 6 else 64)) for i in range(8)]).astype(np.uint32)
    if random_table:
        entries, words = [], []
        for _ in range(int(rng.integers(1, 12))):
            mode = int(rng.integers(0, 5))
            linear = bool(rng.integers(0, 2))
            ps = []
            for _ in range(int(rng.integers(1, 4))):
                leaf = int(rng.integers(0, 8))
                w = 256 if leaf < 6 else 64
                ln = int(rng.integers(1, w + 1))
                ps.append((leaf, int(rng.integers(0, w - ln + 1)), int(rng.integers(0, 257 - ln)), ln))
            truth = 0 if mode == XOR else int(rng.integers(0, 2)) if rng.integers(0, 2) else \
                RP.BOUND_ATOM | int(rng.integers(0, 3))
            fixed = _rand(rng) if mode != XOR or linear else 0
            entries.append((int(rng.integers(0, 3)), ps, mode, truth, fixed))
            words.append((int(rng.choice([-1, 1])), int(rng.integers(0, 2)) if mode == XOR else 0)
                         if linear else None)
    else:
        entries = [(0, [(0, 0, 0, 256)], XOR, 0, 0), (0, [(1, 0, 0, 256)], XOR, 0, 0),
                   (1, [(2, 0, 0, 256)], LOW, 0, 0), (1, [(3, 0, 0, 256)], LOW_S, 1, 0),
                   (2, [(4, 0, 0, 256)], HIGH, RP.BOUND_ATOM | 0, 0),
                   (2, [(5, 0, 0, 256)], HIGH_S, RP.BOUND_ATOM | 2, 0),
                   (0, [(6, 0, 8, 64)], XOR, 0, 0x55), (1, [(7, 4, 0, 60)], HIGH, 0, 0xF << 60),
                   (0, [(0, 0, 128, 128), (0, 128, 0, 128)], XOR, 0, 0),
                   (0, [(2, 0, 0, 256)], XOR, 0, 0),
                   (1, [(1, 0, 0, 256)], LOW, 1, 0), (2, [(3, 3, 5, 100)], HIGH_S, 0, 0x1F)]
        words = [(1, 0), (-1, 1), (1, 0), (-1, 0), (1, 0), (-1, 0), (-1, 1), (1, 0), (1, 1), None,
                 None, (-1, 0)]
    B = RP.make_bounds(entries, 2, 3)
    S = RP.make_sums(words, 2)
    rv = np.stack([_row(_rand(rng)) for _ in range(3)]).astype(np.uint32)
    sv = np.stack([_row(_rand(rng)) for _ in range(2)]).astype(np.uint32)
    return gens, base, B, S, rv, sv


def _state(rng, rv, sv, all_live=False):
    roots = np.zeros(2, bool) if all_live else rng.integers(0, 2, 2).astype(bool)
    atoms = np.zeros(3, bool) if all_live else rng.integers(0, 2, 3).astype(bool)
    return rv, roots, atoms, np.zeros(0, np.uint32), sv


@pytest.mark.parametrize("random_table", [False, True])
def test_library_lanes_equal_the_specification_on_synthetic_tables(random_table):
    rng = np.random.default_rng(0x73756D + random_table)
    consts = np.zeros((1, 8), dtype=np.uint32)
    U = RP.no_ufs()
    linear = 0
    for it in range(12 if random_table else 4):
        gens, base, B, S, rv, sv = synthetic(rng, random_table)
        state = _state(rng, rv, sv, all_live=it == 0)
        for r, lanes in ((1, 16), (2, 257), (3, 4096)):
            spec = RP.sum_mutate_ref(gens, consts, base, state, B, S, 77, r, lanes)
            lib, moves = walk_sum_mutate_host(gens, consts, base, state, B, U, S, 77, r, lanes)
            assert np.array_equal(spec, lib)
            picks = RP.uf_picks_ref(state, B, r, lanes)
            assert np.array_equal(moves[:, 4].astype(np.int64), picks)
            linear += sum(1 for e in picks if e != NONE and S.lin[int(e)])
        spec = RP.sum_mutate_ref(gens, consts, base, None, B, S, 77, 0, 64)
        lib, moves = walk_sum_mutate_host(gens, consts, base, None, B, U, S, 77, 0, 64)
        assert np.array_equal(spec, lib) and (moves[:, 4] == NONE).all()
    assert linear > 50


def test_a_linear_move_changes_the_side_by_what_it_must():
    """The arithmetic, in integers: with S = X - Y + c, each mode's move on
    either target gives the side the value the mode names."""
    rng = np.random.default_rng(5)
    gens = [LeafGen(256, 0, 0, 0, 0, 0)] * 2
    consts = np.zeros((1, 8), dtype=np.uint32)
    M = RP.M256
    for mode in range(5):
        for target, sign in ((0, 1), (1, -1)):
            x, y, c, other = (_rand(rng) for _ in range(4))
            side = (x - y + c) & M
            resid = side ^ other if mode == XOR else (side - other if mode <= LOW_S else other - side) & M
            B = RP.make_bounds([(0, [(target, 0, 0, 256)], mode, 0, 0)], 1, 0)
            S = RP.make_sums([(sign, 0)], 1)
            state = (_row(resid)[None], np.zeros(1, bool), np.zeros(0, bool),
                     np.zeros(0, np.uint32), _row(side)[None])
            base = np.stack([_row(x), _row(y)]).astype(np.uint32)
            out, moves = walk_sum_mutate_host(gens, consts, base, state, B, RP.no_ufs(), S, 1, 1, 16)
            assert moves[1, 4] == 0 and moves[1, 0] == 0          # lane 1: the aim alone
            x2, y2 = RP._ints(np.ascontiguousarray(out[:, :, 1]))
            s = 1 if mode in (LOW_S, HIGH_S) else 0
            want = other if mode == XOR else (other - s if mode <= LOW_S else other + s) & M
            assert (x2 - y2 + c) & M == want
            assert (x2, y2)[1 - target] == (x, y)[1 - target]


def test_a_leaf_a_plain_move_owns_is_skipped_and_dst_may_be_the_base():
    """Lanes n1 + 1 .. 2 n1 take their plain moves over the aimed result: a
    move on the target's leaf wins.  mg_walk_sum_mutate_host writes apart
    from the base; the adopt path writes in place, which the stand-alone fuzz
    program compares (tests/fuzz_walk_sum.cpp)."""
    rng = np.random.default_rng(9)
    gens, base, B, S, rv, sv = synthetic(rng)
    gens = [LeafGen(g.width, 0, 0, 50, 70, 85) for g in gens]
    consts = np.zeros((1, 8), dtype=np.uint32)
    state = _state(rng, rv, sv, all_live=True)
    owned = 0
    for r in range(1, 6):
        spec = RP.sum_mutate_ref(gens, consts, base, state, B, S, 3, r, 4096)
        lib, moves = walk_sum_mutate_host(gens, consts, base, state, B, RP.no_ufs(), S, 3, r, 4096)
        assert np.array_equal(spec, lib)
        for j in np.flatnonzero((moves[:, 4] != NONE) & (moves[:, 0] > 0)):
            e = int(moves[j, 4])
            mine = {int(moves[j, 2])} | ({int(moves[j, 3])} if moves[j, 0] > 1 else set())
            owned += bool(S.lin[e]) and bool(mine & {l for l, *_ in B.of(e)})
    assert owned > 0


@pytest.mark.parametrize("name", SC.NAMES)
def test_library_equals_the_specification_on_the_cases(name):
    prog = SC.program(name)
    B, U, S = SC.tables(name)
    gens, consts = default_leafgen(prog), SC.consts_of(prog)
    res = SC.reference(name)
    for base in (SC.start_rows(name), np.asarray(res.leaves[0])):
        bits, abits, resid, urows, srows = SC.values_fn(name)(np.ascontiguousarray(base[:, :, None]))
        state = (resid[:, :, 0], bits[0], abits[0], RP.uf_resolve_ref(base, urows[:, :, 0], U),
                 srows[:, :, 0])
        for r, lanes in ((1, 16), (2, 300)):
            spec = RP.sum_mutate_ref(gens, consts, base, state, B, S, SC.SEED, r, lanes)
            lib, _ = walk_sum_mutate_host(gens, consts, base, state, B, U, S, SC.SEED, r, lanes)
            assert np.array_equal(spec, lib)


@pytest.mark.parametrize("name", UC.NAMES)
def test_without_a_linear_entry_it_is_the_lane_function_of_uf(name):
    prog = UC.program(name)
    B, U = UC.tables(name)
    gens, consts = default_leafgen(prog), UC.consts_of(prog)
    base = UC.start_rows(name)
    bits, abits, resid, urows = UC.values_fn(name)(np.ascontiguousarray(base[:, :, None]))
    state = (resid[:, :, 0], bits[0], abits[0], RP.uf_resolve_ref(base, urows[:, :, 0], U))
    none = RP.no_sums(len(B))
    for r, lanes in ((1, 64), (3, 257)):
        want, wm = walk_uf_mutate_host(gens, consts, base, state, B, U, UC.SEED, r, lanes)
        got, gm = walk_sum_mutate_host(gens, consts, base, state + (np.zeros((0, 8), np.uint32),),
                                       B, U, none, UC.SEED, r, lanes)
        assert np.array_equal(want, got) and np.array_equal(wm, gm)
        assert np.array_equal(RP.sum_mutate_ref(gens, consts, base, state + ([],), B, none,
                                                UC.SEED, r, lanes),
                              RP.uf_mutate_ref(gens, consts, base, state, B, UC.SEED, r, lanes))


# ---------------------------------------------------------------------------
# the validator
# ---------------------------------------------------------------------------

def _refused(gens, base, B, S, state, U=None):
    with pytest.raises(EngineError):
        walk_sum_mutate_host(gens, np.zeros((1, 8), np.uint32), base, state, B,
                             RP.no_ufs() if U is None else U, S, 1, 1, 16)


def test_malformed_lin_words_are_refused():
    rng = np.random.default_rng(2)
    gens, base, B, S, rv, sv = synthetic(rng)
    state = _state(rng, rv, sv)
    walk_sum_mutate_host(gens, np.zeros((1, 8), np.uint32), base, state, B, RP.no_ufs(), S, 1, 1, 16)

    def with_lin(e, w, n_srows=2):
        lin = np.array(S.lin, copy=True)
        lin[e] = w
        return RP.Sums(lin, n_srows)
    _refused(gens, base, B, with_lin(0, 2), state)                   # NEG without LINEAR
    _refused(gens, base, B, with_lin(0, 1 | 4), state)               # an unknown bit
    _refused(gens, base, B, with_lin(0, 1 | 1 << 16), state)
    _refused(gens, base, B, with_lin(0, 1 | 2 << 8), state)          # a side row at n_srows
    _refused(gens, base, B, with_lin(1, 1 | 1 << 8, 1), state)
    _refused(gens, base, B, with_lin(2, 1 | 1 << 8), state)          # a row in an order entry
    _refused(gens, base, B, RP.Sums(np.array(S.lin), 65), state)     # more than 64 rows
    # a slot piece in a linear entry
    U = RP.make_ufs(slots=[(0, 0)], funcs=[(0, 1, 1)], cands=[(0, RP.UF_ALWAYS, 0, 0, 0, 0)],
                    n_urows=1)
    ust = state[:3] + (np.array([0], np.uint32), state[4])
    slot = RP.make_bounds([(0, [(RP.UF_SLOT | 0, 0, 0, 256)], XOR, 0, 0)], 2, 3)
    walk_sum_mutate_host(gens, np.zeros((1, 8), np.uint32), base, ust, slot, U, RP.no_sums(1), 1, 1, 16)
    _refused(gens, base, slot, RP.make_sums([(1, 0)], 2), ust, U)
    # a fixed word in an XOR entry that is not linear stays refused, as in mg_walk_uf
    fx = RP.make_bounds([(0, [(0, 0, 0, 256)], XOR, 0, 5)], 2, 3)
    _refused(gens, base, fx, RP.no_sums(1), state)
    walk_sum_mutate_host(gens, np.zeros((1, 8), np.uint32), base, state, fx, RP.no_ufs(),
                         RP.make_sums([(1, 0)], 2), 1, 1, 16)
    # what mg_walk_uf_ok refuses for any entry: a piece past its leaf, a residual out of range
    bad = RP.make_bounds([(0, [(6, 8, 0, 64)], XOR, 0, 5)], 2, 3)
    _refused(gens, base, bad, RP.make_sums([(1, 0)], 2), state)
    bad = RP.make_bounds([(3, [(0, 0, 0, 256)], XOR, 0, 5)], 2, 3)
    _refused(gens, base, bad, RP.make_sums([(1, 0)], 2), state)


def test_null_tables_with_counts_are_refused():
    import ctypes as C
    from mythril_amd.engine import _ptr, load_library
    lib = load_library()
    gens = (LeafGen * 1)(LeafGen(256, 0, 0, 0, 0, 0))
    base, out = np.zeros((1, 8), np.uint32), np.zeros((1, 8, 4), np.uint32)
    entries = np.array([[0, 0, 1, 0, 0]], np.uint32)
    pieces = np.array([[0, 0, 0, 256]], np.uint32)
    fixed, lin = np.zeros((1, 8), np.uint32), np.zeros(1, np.uint32)

    def call(e, p, f, l):
        return lib.mg_walk_sum_mutate_host(
            C.cast(gens, C.c_void_p), 1, None, 0, _ptr(base), None, 1, None, 1, 0, e, 1, p, 1, f, l,
            None, 0, None, 0, None, 0, None, 0, None, 0, 0, None, 1, 0, 4, 0, 4, _ptr(out), None)
    assert call(_ptr(entries), _ptr(pieces), _ptr(fixed), _ptr(lin)) == 0
    assert call(_ptr(entries), _ptr(pieces), _ptr(fixed), None) != 0
    assert call(None, _ptr(pieces), _ptr(fixed), _ptr(lin)) != 0
    assert call(_ptr(entries), None, _ptr(fixed), _ptr(lin)) != 0
    assert call(_ptr(entries), _ptr(pieces), None, _ptr(lin)) != 0

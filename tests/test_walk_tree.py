"""The tree-scored walk without a GPU: every rewriting rule
of repair.distance_trees on small symbols against oracle/smtlib_ref.py, with
the distance recomputed independently from Python ints; the library's scoring
(csrc/mg_walk_tree.h through mg_walk_tree_score_host) against its numpy
specification (repair.tree_score_ref) at the sizes where its paths change;
the validator's refusals; the trees of the two known misses; and the
conditions on the crafted cases (tests/tree_cases.py): the generator finds no
model, the walk under today's residual table stays stuck, the tree walk
reaches a model within half of the round budget."""

import json
import os
import types

import numpy as np
import pytest

import tree_cases as K
import walk_cases as WK
from mythril_amd import repair as RP
from mythril_amd.engine import EngineError, walk_score_host, walk_tree_score_host
from mythril_amd.smt import node as N
from oracle import smtlib_ref as R
from test_walk import pack_masks, rows_of, score_inputs

FLAT, HAMMING, MAGNITUDE = RP.FLAT, RP.HAMMING, RP.MAGNITUDE
ATOM, AND, OR, INF, END = RP.WT_ATOM, RP.WT_AND, RP.WT_OR, RP.WT_PUSH_INF, RP.WT_END
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------
# the crafted cases
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.NAMES)
def test_crafted_cases_need_the_tree(name):
    """The conditions on the inputs, none of them a measurement: (a) the
    generator finds no model among lanes x max_rounds candidates, (b) walk_ref
    under today's residuals() table is still failing after max_rounds from the
    same start, (c) the tree walk reaches a model within half of max_rounds."""
    rounds = K.MAX_ROUNDS[name]
    tree, table = K.program(name), K.program(name, 16, "table")
    assert [l.source for l in tree.leaves] == [l.source for l in table.leaves]
    assert tree.const_values == table.const_values            # the same moves on both
    T = K.trees(name)
    assert T.is_tree(0) and not any(T.is_tree(k) for k in range(1, len(T.roots)))
    assert int(K.table_scoring(name)[1][0]) == FLAT << 16     # today: no distance
    kinds = sorted(int(a) >> 16 for a in T.atoms)
    assert kinds == {"chain": [FLAT, HAMMING], "conj": [HAMMING, MAGNITUDE, MAGNITUDE],
                     "nest": [HAMMING, HAMMING, HAMMING, MAGNITUDE, MAGNITUDE]}[name]
    start = K.start_rows(name)
    bits = K.bits_fn(name)
    assert (~bits(start[:, :, None])[0]).tolist() == [True] + [False] * (len(T.roots) - 1)
    assert K.generator_hits(name, K.LANES * rounds) == 0                          # (a)
    stuck = K.table_reference(name)
    assert stuck.nfail[0] > 0 and stuck.rounds == rounds                          # (b)
    assert (stuck.trace[0, :, 0] == 1).all() and (stuck.trace[0, :, 1] == 1).all()
    res = K.reference(name)
    zero = np.flatnonzero(res.trace[0, :res.rounds, 0] == 0)
    assert zero.size and int(zero[0]) < rounds // 2                               # (c)
    assert int(zero[0]) == K.FIRST_ZERO[name]                 # what the cases' docstring says
    assert res.nfail[0] == 0 == res.cost[0] and res.winner == 0 and res.rounds % 8 == 0
    assert bits(np.asarray(res.leaves[0])[:, :, None])[0].all()
    keys = res.trace[0, :res.rounds].astype(np.int64)
    keys = keys[:, 0] << 20 | keys[:, 1]
    assert (np.diff(keys) <= 0).all() and (np.diff(keys) < 0).sum() >= 8          # a descent


def test_default_walk_ref_is_unchanged_by_the_scoring_argument():
    """score=None is today's loop; a score that wraps the table scoring gives
    the same walk."""
    name = "magnitude"
    prog = WK.program(name)
    table = WK.scoring(name)[1]
    args = (WK.values_fn(name), WK.default_leafgen(prog), WK.consts_of(prog), WK.starts(name, 2),
            table, WK.SEED, 256, 8)
    want = WK.reference(name, 2, 256, 8)
    got = RP.walk_ref(*args, score=lambda bits, resid: RP._score_bits(bits, resid, table))
    for a, b in ((got.leaves, want.leaves), (got.nfail, want.nfail), (got.cost, want.cost),
                 (got.trace, want.trace)):
        assert np.array_equal(a, b)
    assert got.rounds == want.rounds and got.winner == want.winner


# ---------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------

def rule_roots():
    """(name, constraint, expected shape) for every rule of §3.11 over small
    symbols.  Shape: nested tuples of 'and' / 'or' with atom kinds F, H, M at
    the leaves; 'simple:K' for a root stored as a simple entry of kind K."""
    a, b, c, d = (N.bv_var("r" + s, 8) for s in "abcd")
    p, q = N.bool_var("rp"), N.bool_var("rq")
    n8 = lambda v: N.bv_num(v, 8)
    lt, le = N.bv_cmp("bvult", a, b), N.bv_cmp("bvsle", c, d)
    eq, eq2 = N.eq(a, b), N.eq(c, n8(7))
    no = lambda x: N.bool_op("not", x)
    F, H, M = "F", "H", "M"
    arr = N.array_var("rA", 8, 8)
    chain_k = N.store(N.store(N.const_array(8, n8(0)), a, c), b, d)
    chain_a = N.store(arr, a, c)
    f = lambda x: N.apply_uf("rf", 8, 8, x)
    wide_a = N.concat(N.bv_var("w0", 100), N.bv_var("w1", 100), N.bv_var("w2", 100))
    wide_b = N.concat(N.bv_var("w3", 150), N.bv_var("w4", 150))
    word = lambda x: N.ite(x, N.bv_num(1, 256), N.bv_num(0, 256))
    rows = [
        ("and", N.bool_op("and", eq, lt, p), ("and", H, M, F)),
        ("or", N.bool_op("or", eq, lt, p), ("or", H, M, F)),
        ("implies", N.bool_op("=>", eq, lt), ("or", F, M)),
        ("not implies", no(N.bool_op("=>", eq, lt)), ("and", H, M)),
        ("bool ite", N.ite(p, eq, lt), ("or", ("and", F, H), ("and", F, M))),
        ("not bool ite", no(N.ite(p, eq, lt)), ("or", ("and", F, F), ("and", F, M))),
        ("de morgan and", no(N.bool_op("and", eq, lt)), ("or", F, M)),
        ("de morgan or", no(N.bool_op("or", eq, le, p)), ("and", F, M, F)),
        ("nested", N.bool_op("and", eq, N.bool_op("or", lt, N.bool_op("and", le, eq2))),
         ("and", H, ("or", M, ("and", M, H)))),
        ("flattened", N.bool_op("and", eq, N.bool_op("and", lt, le)), ("and", H, M, M)),
        ("laser words", N.bool_op("and", N.eq(word(eq), N.bv_num(1, 256)),
                                  N.eq(word(lt), N.bv_num(0, 256))), ("and", H, M)),
        ("true under and", N.bool_op("and", eq, N.bool_val(True), lt), ("and", H, M)),
        ("false under or", N.bool_op("or", eq, N.bool_val(False), lt), ("or", H, M)),
        ("false under and", N.bool_op("or", lt, N.bool_op("and", eq, N.bool_val(False))),
         "simple:M"),
        ("true under or", N.bool_op("and", lt, N.bool_op("or", eq, N.bool_val(True))),
         "simple:M"),
        ("bool xor", N.bool_op("and", N.bool_op("xor", p, q), eq), ("and", F, H)),
        ("bool eq", N.bool_op("and", N.eq(p, q), eq), ("and", F, H)),
        ("distinct", N.bool_op("and", N.distinct(a, b), eq2), ("and", F, H)),
        ("bv ite left", N.eq(N.ite(p, a, b), c), ("or", ("and", F, H), ("and", F, H))),
        ("bv ite right, negative", no(N.eq(c, N.ite(lt, a, n8(3)))),
         ("or", ("and", M, F), ("and", M, F))),
        ("bv ite numerals", N.eq(N.ite(lt, n8(1), n8(2)), n8(2)), "simple:M"),
        ("store chain on K", N.eq(N.select(chain_k, N.bv_var("rj", 8)), n8(5)),
         ("or", ("and", H, H), ("and", F, H, H))),
        ("store chain on K, negative", no(N.eq(N.select(chain_k, N.bv_var("rj", 8)), n8(0))),
         ("or", ("and", H, F), ("and", F, H, F))),
        ("store chain on an array", N.eq(N.select(chain_a, b), d),
         ("or", ("and", H, H), ("and", F, H))),
        ("numerals", N.bool_op("and", N.eq(n8(3), n8(3)), eq), "simple:H"),
        ("congruence", N.eq(f(a), f(N.bv_op("bvadd", b, c))), ("or", H, H)),
        ("other UF", N.eq(f(a), N.apply_uf("rg", 8, 8, b)), "simple:H"),
        ("wide", N.eq(wide_a, wide_b), ("and", H, H)),
        ("wide numerals", N.eq(N.concat(a, N.bv_num(5, 256)), N.concat(b, N.bv_num(5, 256))),
         "simple:H"),
        ("one bit", N.bool_op("and", N.eq(N.extract(0, 0, a), N.bv_num(1, 1)), eq),
         ("and", F, H)),
        ("negative equality", no(eq), "simple:F"),
        ("positive equality", eq, "simple:H"),
        ("order", lt, "simple:M"),
        ("negated order", no(lt), "simple:M"),
        ("negated signed order", N.bool_op("and", no(le), p), ("and", M, F)),
        ("wide order", N.bv_cmp("bvult", wide_a, wide_b), "simple:F"),
        ("variable", p, "simple:F"),
    ]
    return rows


def shape_of(T, k):
    names = {FLAT: "F", HAMMING: "H", MAGNITUDE: "M"}
    if not T.is_tree(k):
        return "simple:" + names[T.kind(k)]

    def walk(t):
        if t[0] == "atom":
            return names[int(T.atoms[t[1]]) >> 16]
        return (t[0],) + tuple(walk(c) for c in t[1])
    return walk(T.shapes[k])


def independent_distance(T, k, atom_true, resid_vals):
    """Root k's distance from Python ints and the tree itself (not its code):
    and = sum saturating at 1023, or = min."""
    def entry(e):
        kind, p = int(e) >> 16, int(e) & 0xFFFF
        return 1 if kind == FLAT else max(1, bin(resid_vals[p]).count("1")) if kind == HAMMING \
            else 1 + resid_vals[p].bit_length()

    if not T.is_tree(k):
        return entry(T.roots[k])

    def walk(t):
        if t[0] == "atom":
            return 0 if atom_true[t[1]] else entry(T.atoms[t[1]])
        if t[0] == "false":
            return 1023
        vals = [walk(c) for c in t[1]]
        return min(1023, sum(vals)) if t[0] == "and" else min(vals)
    return walk(T.shapes[k])


def random_assignment(nodes, rng):
    """Random values, small ones often (equalities and hits do hold); every
    array and UF a small table."""
    vars_, arrays, funcs = {}, {}, {}
    for n in N.topo_order(nodes):
        if n.op == "var":
            w = 1 if n.is_bool() else n.width
            v = int.from_bytes(rng.bytes(40), "little") & ((1 << w) - 1)
            vars_[n.params[0]] = v if rng.integers(3) == 0 else v & 3
        elif n.op == "array":
            arrays[n.params[0]] = ([(int(k), int(rng.integers(4))) for k in range(4)],
                                   int(rng.integers(4)))
        elif n.op == "apply":
            funcs[n.params[0]] = ([(int(k), int(rng.integers(3))) for k in range(6)],
                                  int(rng.integers(3)))
    return R.Assignment(vars_, arrays, funcs)


@pytest.mark.parametrize("seed", range(3))
def test_every_rule_against_the_oracle(seed):
    rng = np.random.default_rng(seed)
    rows = rule_roots()
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    cs = [r[1] for r in rows]
    T = RP.distance_trees(cs)
    for k, (name, _, want) in enumerate(rows):
        assert shape_of(T, k) == want, name
    assert len({n.id for n in T.atom_nodes}) == T.n_atoms           # shared by (node, polarity)
    assert len({p.id for p in T.probes}) == T.n_resid               # one probe per term
    assert all(p.is_bv() and p.width <= 256 for p in T.probes)
    assert all(n.is_bool() for n in T.atom_nodes)
    n = 64
    bits = np.zeros((n, len(cs)), dtype=bool)
    abits = np.zeros((n, T.n_atoms), dtype=bool)
    resid = [[0] * n for _ in T.probes]
    want_cost = np.zeros(n, dtype=np.int64)
    zero_when_true = np.zeros(len(cs), dtype=int)
    for a in range(n):
        asg = random_assignment(cs + T.atom_nodes, rng)
        holds = R.evaluate(cs, asg)
        atom_true = [bool(v) for v in R.evaluate(T.atom_nodes, asg)]
        vals = R.evaluate(T.probes, asg)
        for i, v in enumerate(vals):
            resid[i][a] = v
        abits[a] = atom_true
        for k, (name, c, _) in enumerate(rows):
            bits[a, k] = bool(holds[k])
            d = independent_distance(T, k, atom_true, vals)
            if T.is_tree(k):                   # 0 exactly when the root holds
                assert (d == 0) == bool(holds[k]), (name, d)
                zero_when_true[k] += d == 0
            elif T.kind(k) == HAMMING:         # the mask and the residual agree
                assert (vals[int(T.roots[k]) & 0xFFFF] == 0) == bool(holds[k]), name
            if not holds[k]:
                want_cost[a] += min(1023, max(1, d))
    trees_ = [k for k in range(len(cs)) if T.is_tree(k)]
    assert len(trees_) >= 20 and (zero_when_true[trees_] > 0).sum() > len(trees_) // 2
    assert (~bits).any(axis=0).sum() > len(cs) // 2                 # roots do fail
    args = (pack_masks(bits), pack_masks(abits), rows_of(resid, n), T, len(cs))
    nfail, cost = RP.tree_score_ref(*args)
    assert np.array_equal(nfail, (~bits).sum(axis=1)) and np.array_equal(cost, want_cost)
    assert (cost >= nfail).all() and not cost[nfail == 0].any()
    nf, co = walk_tree_score_host(*args)
    assert np.array_equal(nf, nfail) and np.array_equal(co, cost)


def test_negated_order_is_the_opposite_order():
    a, b = N.bv_var("na", 16), N.bv_var("nb", 16)
    for op, back in (("bvult", "bvuge"), ("bvule", "bvugt"), ("bvugt", "bvule"),
                     ("bvuge", "bvult"), ("bvslt", "bvsge"), ("bvsle", "bvsgt"),
                     ("bvsgt", "bvsle"), ("bvsge", "bvslt")):
        T = RP.distance_trees([N.bool_op("not", N.bv_cmp(op, a, b))])
        assert shape_of(T, 0) == "simple:M" and T.n_atoms == 0 and len(T.code) == 0
        # not (a < b) is b <= a: R = b - a, signedness kept
        x, y = (b, a) if op in ("bvult", "bvule", "bvslt", "bvsle") else (a, b)
        assert T.probes[0] is N.bv_op("bvsub", x, y)
        # today's table leaves it flat; a positive order is the same on both
        assert int(RP.residuals([N.bool_op("not", N.bv_cmp(op, a, b))])[1][0]) == FLAT << 16
        pos = [N.bv_cmp(back, a, b)]
        assert np.array_equal(RP.distance_trees(pos).roots, RP.residuals(pos)[1])
        assert RP.distance_trees(pos).probes[0] is T.probes[0]


def test_constraints_without_structure_degenerate_to_the_table():
    for name in ("hamming", "magnitude", "mixed"):
        with N.fresh_scope():
            cs, _ = WK._case(name)
            T = RP.distance_trees(cs)
            probes, table = RP.residuals(cs)
        assert np.array_equal(T.roots, table) and T.n_atoms == 0 and len(T.code) == 0
        assert [p.id for p in T.probes] == [p.id for p in probes]


def test_budgets_collapse_a_subterm_to_one_flat_atom():
    xs = [N.bv_var("g%d" % i, 8) for i in range(80)]
    eqs = [N.eq(xs[2 * i], xs[2 * i + 1]) for i in range(40)]
    # 33 atoms under one and: the and itself is one FLAT atom, the root simple
    T = RP.distance_trees([N.bool_op("and", *eqs[:33])])
    assert shape_of(T, 0) == "simple:F" and T.n_atoms == 0
    # 32 fit: 32 atoms, 63 words and END
    T = RP.distance_trees([N.bool_op("and", *eqs[:32])])
    assert T.is_tree(0) and T.n_atoms == 32 and len(T.code) == 64
    # the oversized subterm collapses, the rest of the root keeps its distance
    big = N.bool_op("or", *eqs[:33])
    T = RP.distance_trees([N.bool_op("and", eqs[39], big)])
    assert shape_of(T, 0) == ("and", "H", "F") and T.atom_nodes[1] is big
    # depth: nine levels of alternating and / or keep eight
    t = eqs[0]
    for i in range(1, 10):
        t = N.bool_op("and" if i % 2 else "or", eqs[i], t)
    T = RP.distance_trees([t])

    def depth(s):
        return 1 if s[0] == "atom" else 1 + max(depth(c) for c in s[1])
    assert T.is_tree(0) and depth(T.shapes[0]) == RP.ROOT_DEPTH
    assert FLAT in [int(a) >> 16 for a in T.atoms]
    assert ok(T)
    # atoms are shared across roots; past 1024 atoms the remaining roots are simple
    ys = [N.bv_var("m%d" % i, 8) for i in range(2200)]
    pairs = [N.bool_op("and", N.eq(ys[2 * i], ys[2 * i + 1]), N.eq(ys[2 * i], N.bv_num(1, 8)))
             for i in range(1100)]
    T = RP.distance_trees(pairs[:3] + pairs[:3])
    assert T.n_atoms == 6 and all(T.is_tree(k) for k in range(6))
    T = RP.distance_trees(pairs[:600])
    assert T.n_atoms == 1024 and [T.is_tree(k) for k in range(600)] == [True] * 512 + [False] * 88
    assert ok(T)


def ok(T, n_resid=None):
    """The library's validator accepts the tables (one all-true lane)."""
    n_roots = len(T.roots)
    masks = pack_masks(np.ones((1, n_roots), dtype=bool))
    amasks = pack_masks(np.ones((1, max(1, len(T.atoms))), dtype=bool))
    n_resid = len(T.probes) if n_resid is None else n_resid
    resid = np.zeros((max(1, n_resid), 8, 1), dtype=np.uint32)
    nf, co = walk_tree_score_host(masks, amasks, resid, T, n_roots, n_resid)
    return nf[0] == 0 == co[0]


@pytest.mark.parametrize("wl,qi,ci", [("c4", 16, 26), ("c3o", 50, 22)])
def test_the_known_misses_get_a_gradient(wl, qi, ci):
    """The blocking roots of the two known misses (tests/golden/
    recall_known_miss.json and c3o query 50): FLAT under
    residuals(), a tree with HAMMING or MAGNITUDE atoms within the budgets
    here."""
    from mythril_amd import workloads as W
    n = json.load(open(os.path.join(GOLDEN, "recall_labels.json")))["n"]
    q = W.queries(wl, max(n, qi + 1))[qi]
    assert int(RP.residuals([q[ci]])[1][0]) == FLAT << 16
    T = RP.distance_trees([q[ci]])
    assert T.is_tree(0)
    kinds = [int(a) >> 16 for a in T.atoms]
    assert HAMMING in kinds or MAGNITUDE in kinds
    assert 1 <= T.n_atoms <= RP.ROOT_ATOMS and len(T.code) <= RP.ROOT_WORDS
    assert ok(T)
    if wl == "c4":            # the congruence arm: the calldata word against the earlier hash
        assert any(a.op == "=" and {x.op for x in a.args} == {"apply", "concat"}
                   for a in T.atom_nodes)
    whole = RP.distance_trees(q)            # the whole query stays within the limits too
    assert whole.n_atoms <= RP.MAX_ATOMS and whole.is_tree(ci) and ok(whole)


# ---------------------------------------------------------------------------
# the library against the specification
# ---------------------------------------------------------------------------

def tables(roots, atoms, code):
    return types.SimpleNamespace(roots=np.array(roots, dtype=np.uint32),
                                 atoms=np.array(atoms, dtype=np.uint32),
                                 code=np.array(code, dtype=np.uint32), probes=[],
                                 n_atoms=len(atoms), n_resid=0)


def random_program(rng, n_atoms, budget):
    """A random valid postfix program (without END): (words, atoms used,
    stack needed).  n-ary AND / OR words, INF arms, nesting."""
    def node(level, room):
        if n_atoms and (level >= 3 or room <= 1 or rng.integers(3) == 0):
            return [ATOM << 16 | int(rng.integers(n_atoms))], 1, 1
        if not n_atoms or rng.integers(8) == 0:
            return [INF << 16], 0, 1
        n = int(rng.integers(1, min(5, room) + 1))
        words, used, stack = [], 0, 0
        for i in range(n):
            w, u, s = node(level + 1, max(1, room // n))
            words += w
            used += u
            stack = max(stack, i + s)
        return words + [(AND if rng.integers(2) else OR) << 16 | n], used, stack
    while True:
        words, used, stack = node(0, budget)
        if used <= RP.ROOT_ATOMS and len(words) < RP.ROOT_WORDS and stack <= RP.WT_STACK:
            return words


def random_tables(n_roots, n_atoms, n_resid, seed):
    rng = np.random.default_rng(seed)

    def entry():
        kind = int(rng.integers(3)) if n_resid else FLAT
        return kind << 16 | (int(rng.integers(n_resid)) if kind != FLAT else 0)
    atoms = [entry() for _ in range(n_atoms)]
    roots, code = [], []
    for k in range(n_roots):
        if rng.integers(3) == 0:
            roots.append(entry())
            continue
        roots.append(RP.WT_TREE | len(code))
        code += random_program(rng, n_atoms, 16) + [END << 16]
    return tables(roots, atoms, code)


@pytest.mark.parametrize("n_roots,n_atoms", [(1, 1), (31, 0), (32, 255), (33, 256), (256, 257),
                                             (257, 1024), (1024, 33)])
def test_library_scores_equal_the_specification(n_roots, n_atoms):
    n = 130
    bits, resid, _ = score_inputs(n_roots, n, n_roots)
    rng = np.random.default_rng(n_atoms)
    abits = rng.random((n, n_atoms)) < 0.5
    T = random_tables(n_roots, n_atoms, resid.shape[0], n_roots + n_atoms)
    assert n_roots == 1 or any(int(r) & RP.WT_TREE for r in T.roots)
    masks, amasks = pack_masks(bits), pack_masks(abits) if n_atoms else None
    # bits at or above n_roots and n_atoms are ignored
    junk = rng.integers(0, 1 << 32, masks.shape, dtype=np.uint32)
    masks = masks | (junk & ~pack_masks(np.ones((n, n_roots), dtype=bool)))
    if n_atoms:
        junk = rng.integers(0, 1 << 32, amasks.shape, dtype=np.uint32)
        amasks = amasks | (junk & ~pack_masks(np.ones((n, n_atoms), dtype=bool)))
    want_nfail, want_cost = RP.tree_score_ref(masks, amasks, resid, T, n_roots)
    nfail, cost = walk_tree_score_host(masks, amasks, resid, T, n_roots)
    assert np.array_equal(nfail, want_nfail) and np.array_equal(cost, want_cost)
    assert nfail[0] == 0 == cost[0] and nfail[1] == n_roots <= cost[1]
    assert np.array_equal(want_nfail, (~bits).sum(axis=1))
    assert int(cost.max()) <= n_roots * 1023 < 1 << 20


def test_the_limits_of_a_program():
    """Depth 8, a 64-word program, a sum that saturates, INF, the clamp at 1."""
    n = 70
    rng = np.random.default_rng(8)
    n_atoms = 40
    atoms = [MAGNITUDE << 16 | i % 4 for i in range(n_atoms)]
    resid = np.zeros((4, 8, n), dtype=np.uint32)
    resid[:, 7, :] = 0x80000000                         # bit length 256: every atom 257 away
    deep = [ATOM << 16 | i for i in range(8)] + [AND << 16 | 8]          # the stack at 8
    long_ = [ATOM << 16]
    for i in range(1, 32):
        long_ += [ATOM << 16 | i, (OR if i % 2 else AND) << 16 | 2]      # 63 words and END
    assert len(long_) == 63
    nest = [ATOM << 16 | 32]
    for i in range(33, 40):                             # and(a, or(b, and(c, ...))): depth 8
        nest = [ATOM << 16 | i] + nest + [(AND if i % 2 else OR) << 16 | 2]
    inf_arm = [INF << 16, ATOM << 16 | 1, OR << 16 | 2]
    only_inf = [INF << 16]
    holds = [ATOM << 16 | 39, AND << 16 | 1]            # value 0 where atom 39 holds: clamped to 1
    progs = [deep, long_, nest, inf_arm, only_inf, holds]
    roots, code = [], []
    for p in progs:
        roots.append(RP.WT_TREE | len(code))
        code += p + [END << 16]
    T = tables(roots, atoms, code)
    bits = np.zeros((n, len(progs)), dtype=bool)
    bits[0] = True
    abits = rng.random((n, n_atoms)) < 0.6
    abits[1] = False
    abits[2] = True
    args = (pack_masks(bits), pack_masks(abits), resid, T, len(progs))
    nfail, cost = RP.tree_score_ref(*args)
    nf, co = walk_tree_score_host(*args)
    assert np.array_equal(nf, nfail) and np.array_equal(co, cost)
    assert nfail[0] == 0 == cost[0]
    one = lambda p: RP.tree_score_ref(args[0], args[1], resid, tables(
        [RP.WT_TREE] + [FLAT << 16] * (len(progs) - 1), atoms, p + [END << 16]), 1)[1]
    assert one(deep)[1] == 1023 and 8 * 257 > 1023              # saturated
    assert one(only_inf)[1] == 1023 and one(inf_arm)[1] == 257 and one(inf_arm)[2] == 1
    assert one(holds)[2] == 1 and one(holds)[1] == 257           # a failing root costs >= 1
    assert one(deep)[2] == 1


def test_all_simple_trees_score_as_the_table():
    for n_roots in (1, 33, 257):
        bits, resid, table = score_inputs(n_roots, 90, n_roots)
        masks = pack_masks(bits)
        want = RP.score_ref(masks, resid, table, n_roots)
        T = RP.simple_trees(table)
        for got in (RP.tree_score_ref(masks, None, resid, T, n_roots),
                    walk_tree_score_host(masks, None, resid, T, n_roots),
                    walk_score_host(masks, resid, table, n_roots)):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_validator_refusals():
    n_resid = 3
    atoms = [HAMMING << 16 | 2, FLAT << 16, MAGNITUDE << 16]
    good = [ATOM << 16, ATOM << 16 | 1, AND << 16 | 2, ATOM << 16 | 2, OR << 16 | 2, END << 16]
    masks = pack_masks(np.zeros((4, 2), dtype=bool))
    amasks = pack_masks(np.zeros((4, 3), dtype=bool))
    resid = np.ones((n_resid, 8, 4), dtype=np.uint32)

    def run(roots, atoms_, code, n_roots=2, nr=n_resid, am=amasks):
        return walk_tree_score_host(masks, am, resid, tables(roots, atoms_, code), n_roots, nr)
    roots = [RP.WT_TREE, HAMMING << 16 | 1]
    nf, co = run(roots, atoms, good)
    assert nf.tolist() == [2] * 4 and co.tolist() == [17] * 4         # min(8 + 1, 226) + 8
    nine = [ATOM << 16] * 9 + [AND << 16 | 9, END << 16]
    atoms33 = [ATOM << 16] * 33
    for i in range(32):
        atoms33 += [AND << 16 | 2]
    words65 = [ATOM << 16] + [AND << 16 | 1] * 63 + [END << 16]
    bad = {
        "unknown opcode": (roots, atoms, [5 << 16] + good),
        "unknown opcode, high bits": (roots, atoms, [0x8001 << 16] + good),
        "atom index": (roots, atoms, [ATOM << 16 | 3] + good[1:]),
        "atom kind": (roots, [3 << 16] + atoms[1:], good),
        "atom residual": (roots, [HAMMING << 16 | 3] + atoms[1:], good),
        "simple root kind": ([RP.WT_TREE, 3 << 16], atoms, good),
        "simple root residual": ([RP.WT_TREE, MAGNITUDE << 16 | 3], atoms, good),
        "offset outside code": ([RP.WT_TREE | len(good), FLAT << 16], atoms, good),
        "offset far outside code": ([RP.WT_TREE | 0x7FFFFFFF, FLAT << 16], atoms, good),
        "underflow": (roots, atoms, [ATOM << 16, AND << 16 | 2, END << 16]),
        "pop nothing": (roots, atoms, [ATOM << 16, AND << 16, END << 16]),
        "empty program": (roots, atoms, [END << 16]),
        "two values at END": (roots, atoms, [ATOM << 16, ATOM << 16 | 1, END << 16]),
        "END with an argument": (roots, atoms, [ATOM << 16, END << 16 | 1]),
        "INF with an argument": (roots, atoms, [INF << 16 | 1, END << 16]),
        "no END": (roots, atoms, good[:-1]),
        "stack of nine": (roots, atoms, nine),
        "33 atoms": (roots, atoms, atoms33 + [END << 16]),
        "65 words": (roots, atoms, words65),
        "no code": (roots, atoms, []),
    }
    for why, (r, a, c) in bad.items():
        with pytest.raises(EngineError, match=r"\(-1\)"):
            run(r, a, c)
            pytest.fail(why)
    assert ok(tables(roots, atoms, [ATOM << 16] + [AND << 16 | 1] * 62 + [END << 16]), n_resid)
    assert ok(tables(roots, atoms, [ATOM << 16] * 8 + [AND << 16 | 8, END << 16]), n_resid)
    with pytest.raises(EngineError):
        run(roots, atoms, good, n_roots=0)
    with pytest.raises(EngineError):                                  # residual kinds, no residuals
        walk_tree_score_host(masks, amasks, None, tables(roots, atoms, good), 2)
    with pytest.raises(EngineError):                                  # 1025 atoms
        walk_tree_score_host(masks, pack_masks(np.zeros((4, 1025), dtype=bool)), resid,
                             tables(roots, [FLAT << 16] * 1025, good), 2)
    with pytest.raises(EngineError):                                  # 1025 roots
        walk_tree_score_host(pack_masks(np.ones((4, 1025), dtype=bool)), amasks, resid,
                             tables([FLAT << 16] * 1025, atoms, good), 1025)
    assert run(roots, atoms, good)[0].tolist() == [2] * 4             # and still scores

"""Test infrastructure of the generated walk cases (tests/test_gen_cases.py,
tests/test_gpu_walk_gen.py): constraint sets past one mask word,
one mask probe and one pass of the grid, their eval-form programs, the
oracle's verdicts, atom verdicts and residual values as the ``values_fn`` of
``walk_ref``, and the reference runs, computed once per (case, walkers, lanes,
rounds, scoring).

Every case is built inside a scope of its own, the distance trees and the
residual table before the masks (a program's schedule follows the node ids,
and a wide mask leaves the compiler's spill budget little room).  Every walker
leaves from a random start of its own (START_SEED), so the lanes of one launch
fail different roots and different atoms.  The counts below are asserted when
a case is built.
  rules      three copies, over fresh symbols of one width each (WIDTHS), of
             and(eq, lt, p), or(eq, lt, p), ite(p, eq, le), not or(eq, le, p),
             and(eq, or(lt, and(le, eq2))), ite(p, a, b) = c, eq2, lt, not eq,
             p, or(a ^ c = d, and(le, not lt)): 33 roots (a second root-mask
             word whose tail mask has one bit), 36 atoms (a second atom-mask
             word), 27 residuals, 21 tree roots, 15 leaves
  flats      90 roots and(p_i, or(q_i, and(r_i, extract(i % 60 + 3, i % 60,
             y_(i % 4)) = 5))), p, q, r Bool symbols, y four 64-bit symbols:
             three root-mask words, 330 atoms (a second atom-mask probe), 60
             residuals, 274 leaves, an OR with two live arms in every root
  ladder_ne  256 roots not (x = 251 i mod 2^16) over one 16-bit x (simple FLAT
             roots, no residual), then the tree root and(p, or(q, and(r, e)),
             e) as root 256, e the 64-bit equality y = not z: a second
             root-mask probe with a tree root in it.  With e = (extract(9, 2,
             y) = 5) under the OR alone the root is at most three moves from
             holding and the walk is over in a round or two; e at the top AND
             is some 32 bits away at a random start and a bit or two nearer
             per round, no pool value and no copy satisfies it, and being the
             same atom twice it needs no second residual probe: with one (a
             second leaf's windows, an xor with a constant, a 16-bit leaf) the
             11-slot layout refuses the tree program ("spill budget exceeded")
  ladder_lt  the same with x <u 65535 - 200 i: simple MAGNITUDE roots, 256
             residual probes, 260 probes in all
  deep       ONE root at the validator's limits and four guards: 32 atoms, a
             64-word program, nesting and(.., or(.., and(.., ..))) to depth 8
             and stack 8, and eight 256-bit equalities x_i = C_i at the top
             AND.  Eight, not the ten of a sum about 1280: a random start is
             then 8 * 128 plus the other atoms, about 1050 with a deviation of
             25, so most lanes saturate at 1023, and a POOL move that lands on
             some C_i (128 less) is below it; with nine or more no single
             lane of a round comes below 1023 and the saturated and the
             unsaturated sum are never seen side by side.  Nothing was refused
             by the compiler on the way: the shape compiles on both layouts

STRIDE is the case of the strided tiles: lanes = 786433 = 3 * 2^18 + 1 is
3073 tiles on 2048 blocks, so blocks 0 .. 1024 take a second tile and the last
tile has one active lane.  Two 128-bit leaves x, y, t = y ^ C:
  root 0  and(x[63:0] = t[63:0], x[127:64] = t[127:64])    a tree, AND(H, H)
  root 1  x[63:0] = t[63:0]                                simple HAMMING
  root 2  or(blk = 3, blk = 0), blk bits 12 and 3 of x ^ t  a tree, OR(H, H)
  root 3  x[15:0] = K                                      simple HAMMING
  root 4  y[31:16] = K'                                    simple HAMMING
The start has bits 3 and 12 of x ^ t wrong and the rest right: roots 0 and 1
fail.  Correcting one of the two bits breaks root 2 and correcting them in x
breaks root 3, so no lane with one move is better than the base, and the only
model among the neighbours flips bits 3 and 12 of y with its two moves: a lane
of the upper half (lanes below lanes // 2 have one move), about 0.75 of them
per round.  (Roots 3 and 4 together keep the two POOL moves x = C, y = 0 from
being better than the base: some 200 lanes of a round make them.)  The aim
table has the entry of root 1's residual on x: from round 1 on the aimed lanes
1 and 2 correct x, fail root 3 and are second best.
STRIDE_SEEDS holds, per kernel, a seed whose adopted lane is at or beyond
2048 * 256, alone at its key, with the round it is adopted in and the lane
(tests/test_gpu_walk_gen.py asserts both from the reference's ingredients).
"""

import functools

import numpy as np

import walk_cases as WK
from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import default_leafgen
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N
from oracle import evalref

SEED = 0x67656E
START_SEED = 0x67656E63
NAMES = ("rules", "flats", "ladder_ne", "ladder_lt", "deep")
TREE_CASES = NAMES                                     # every case has a tree root
ROUNDS = 8
# (lanes, walkers) of the GPU parity test, at ROUNDS rounds
SHAPES = ((63, 2), (65, 3), (256, 64), (1000, 2))
# .. but for the 64 walkers, whose CPU reference takes up to 19 s (flats) and
# 33 s (ladder_lt: 257 residuals per lane) at eight rounds: two rounds there,
# so every walker adopts once and is scored again from its own base; the
# lane, walker and root counts kept.  (ladder_lt: one round, 5 s of reference
# per kernel; its second round would cost as much again, and ladder_ne runs
# the same second root-mask probe through two.)
FEWER_ROUNDS = {(256, 64): {"rules": 2, "flats": 2, "ladder_ne": 2, "ladder_lt": 1, "deep": 2}}
MAX_WALKERS = 64
WIDTHS = (8, 33, 64, 160, 256)
# measured when the cases were first built; asserted in _built
COUNTS = {         # roots, atoms, residuals (trees), tree roots, leaves
    "rules": (33, 36, 27, 21, 15),
    "flats": (90, 330, 60, 90, 274),
    "ladder_ne": (257, 4, 1, 1, 6),
    "ladder_lt": (257, 4, 257, 1, 6),
    "deep": (5, 32, 17, 1, 25),
}

_rng = np.random.default_rng(0x67656E)
RULE_WIDTHS = tuple(int(w) for w in _rng.choice(WIDTHS, size=3, replace=False))
# one limb, a width that is no multiple of 32, and all eight limbs of a residual
assert RULE_WIDTHS == (256, 8, 33), RULE_WIDTHS
_RULE_K = [int.from_bytes(_rng.bytes(32), "little") for _ in range(3)]
_DEEP_C = [int.from_bytes(_rng.bytes(32), "little") for _ in range(8)]
_DEEP_K = [int(v) for v in _rng.integers(1, 1 << 16, size=16)]

# the shape the 11-slot layout refuses (tests/test_gen_cases.py asserts it)
REFUSED = "ladder_ne_two_residuals"
STRIDE = "stride"
STRIDE_LANES = 3 * (1 << 18) + 1
STRIDE_BITS = (3, 12)
_STRIDE_C = int.from_bytes(_rng.bytes(16), "little")
_STRIDE_X = int.from_bytes(_rng.bytes(16), "little")
# kernel -> (seed, the round of the adoption checked, its lane)
STRIDE_SEEDS = {
    "repair": (0x73747200, 0, 602749),
    "walk": (0x73747200, 0, 602749),
    "walk_tree": (0x73747200, 0, 602749),
    "walk_aim": (0x73747205, 1, 648488),
}


def rounds_at(name, shape):
    """The rounds of the GPU parity test of ``name`` at (lanes, walkers)."""
    return FEWER_ROUNDS.get(tuple(shape), {}).get(name, ROUNDS)


def _not(x):
    return N.bool_op("not", x)


def _rules_copy(k, w):
    a, b, c, d = (N.bv_var("r%d%s" % (k, s), w) for s in "abcd")
    p = N.bool_var("r%dp" % k)
    eq, eq2 = N.eq(a, b), N.eq(c, N.bv_num(_RULE_K[k] & ((1 << w) - 1), w))
    lt, le = N.bv_cmp("bvult", a, b), N.bv_cmp("bvsle", c, d)
    return [N.bool_op("and", eq, lt, p), N.bool_op("or", eq, lt, p), N.ite(p, eq, le),
            _not(N.bool_op("or", eq, le, p)),
            N.bool_op("and", eq, N.bool_op("or", lt, N.bool_op("and", le, eq2))),
            N.eq(N.ite(p, a, b), c), eq2, lt, _not(eq), p,
            N.bool_op("or", N.eq(N.bv_op("bvxor", a, c), d), N.bool_op("and", le, _not(lt)))]


def _tail(p, q, r, e):
    return N.bool_op("and", p, N.bool_op("or", q, N.bool_op("and", r, e)))


def _case(name):
    if name == "rules":
        return [c for k, w in enumerate(RULE_WIDTHS) for c in _rules_copy(k, w)]
    if name == "flats":
        ys = [N.bv_var("y%d" % i, 64) for i in range(4)]
        return [_tail(N.bool_var("p%02d" % i), N.bool_var("q%02d" % i), N.bool_var("r%02d" % i),
                      N.eq(N.extract(i % 60 + 3, i % 60, ys[i % 4]), N.bv_num(5, 4)))
                for i in range(90)]
    if name in ("ladder_ne", "ladder_lt", REFUSED):
        x, y = N.bv_var("x", 16), N.bv_var("y", 64)
        if name == REFUSED:       # ladder_ne and a second residual in root 256
            cs = [_not(N.eq(x, N.bv_num(251 * i % (1 << 16), 16))) for i in range(256)]
            e = N.eq(y, N.bv_op("bvnot", N.bv_var("z", 64)))
            w = N.eq(N.extract(63, 48, y), N.bv_var("w", 16))
            return cs + [N.bool_op("and", _tail(N.bool_var("p"), N.bool_var("q"),
                                                N.bool_var("r"), e), e, w)]
        if name == "ladder_ne":
            cs = [_not(N.eq(x, N.bv_num(251 * i % (1 << 16), 16))) for i in range(256)]
        else:
            cs = [N.bv_cmp("bvult", x, N.bv_num(65535 - 200 * i, 16)) for i in range(256)]
        e = N.eq(y, N.bv_op("bvnot", N.bv_var("z", 64)))
        return cs + [N.bool_op("and", _tail(N.bool_var("p"), N.bool_var("q"), N.bool_var("r"), e), e)]
    if name == "deep":
        xs = [N.bv_var("x%d" % i, 256) for i in range(8)]
        u, v = N.bv_var("u", 256), N.bv_var("v", 256)
        f = iter([N.bool_var("f%02d" % i) for i in range(15)])
        k = iter(_DEEP_K)
        at = iter(range(0, 256, 16))
        m = lambda: N.bv_cmp("bvult", N.extract(*_win(next(at)), u), N.bv_num(next(k), 16))
        h = lambda: N.eq(N.extract(*_win(next(at)), v), N.bv_num(next(k), 16))
        t = N.bool_op("and", m(), next(f), next(f), next(f))                       # level 7
        for op in ("or", "and", "or", "and", "or"):                                # levels 6 .. 2
            t = N.bool_op(op, h() if op == "or" else m(), next(f), next(f), t)
        eqs = [N.eq(x, N.bv_num(c, 256)) for x, c in zip(xs, _DEEP_C)]
        root = N.bool_op("and", *eqs, m(), next(f), next(f), m(), h(), t)
        # four guards: neither 16-bit window of x0 is 0 or 0xFFFF
        return [root] + [_not(N.eq(N.extract(*_win(lo), xs[0]), N.bv_num(v, 16)))
                         for lo in (64, 128) for v in (0, 0xFFFF)]
    if name == STRIDE:
        x, y = N.bv_var("x", 128), N.bv_var("y", 128)
        t = N.bv_op("bvxor", y, N.bv_num(_STRIDE_C, 128))
        lo = N.eq(N.extract(63, 0, x), N.extract(63, 0, t))
        hi = N.eq(N.extract(127, 64, x), N.extract(127, 64, t))
        d = N.bv_op("bvxor", x, t)
        b0, b1 = STRIDE_BITS
        blk = N.concat(N.extract(b1, b1, d), N.extract(b0, b0, d))
        return [N.bool_op("and", lo, hi), lo,
                N.bool_op("or", N.eq(blk, N.bv_num(3, 2)), N.eq(blk, N.bv_num(0, 2))),
                N.eq(N.extract(15, 0, x), N.bv_num(_STRIDE_X & 0xFFFF, 16)),
                N.eq(N.extract(31, 16, y), N.bv_num(_stride_y() >> 16 & 0xFFFF, 16))]
    raise KeyError(name)


def _stride_y():
    return _STRIDE_X ^ _STRIDE_C ^ sum(1 << b for b in STRIDE_BITS)


def _win(lo):
    return lo + 15, lo


@functools.lru_cache(maxsize=None)
def _built(name):
    """The case's nodes, built in one order inside a scope of their own."""
    with N.fresh_scope():
        cs = _case(name)
        trees = RP.distance_trees(cs)
        probes, table = RP.residuals(cs)
        mask = CS.mask_probes(cs)
        amask = CS.mask_probes(trees.atom_nodes)
    for a in (trees.roots, trees.atoms, trees.code, table):
        a.setflags(write=False)
    if name in COUNTS:
        n_tree = sum(trees.is_tree(k) for k in range(len(cs)))
        assert (len(cs), trees.n_atoms, trees.n_resid, n_tree) == COUNTS[name][:4], (
            name, len(cs), trees.n_atoms, trees.n_resid, n_tree)
    return cs, mask, amask, trees, tuple(probes), table


def case(name):
    """The constraints."""
    return _built(name)[0]


def trees(name):
    return _built(name)[3]


def table_scoring(name):
    """(residual probe nodes, table) of ``repair.residuals``."""
    return _built(name)[4:]


def _extra(name, scoring):
    cs, _, amask, T, probes, _ = _built(name)
    return {"tree": amask + list(T.probes), "table": list(probes), "mask": []}[scoring]


@functools.lru_cache(maxsize=None)
def program(name, nreg=16, scoring="tree"):
    """The case's eval-form program: root mask, then (``tree``) atom mask and
    the trees' residuals, (``table``) the residuals of ``repair.residuals``, or
    (``mask``) nothing more.  Raises ``ir.Unsupported`` where the compiler
    refuses the shape."""
    cs, mask = _built(name)[:2]
    prog = compile_constraints(cs, mask + _extra(name, scoring), nreg=nreg)
    if name in COUNTS:
        assert len(prog.leaves) == COUNTS[name][4], (name, len(prog.leaves))
    return prog


@functools.lru_cache(maxsize=None)
def start_values(name):
    """Per walker {symbol: value}: MAX_WALKERS random starts from one fixed
    generator, each value masked to its leaf's width (by ``leaf_rows``); the
    strided case has ONE start, the near miss of the module docstring."""
    if name == STRIDE:
        return ({"x": _STRIDE_X, "y": _stride_y()},)
    leaves = sorted((l.source, l.width) for l in program(name).leaves)
    rng = np.random.default_rng([START_SEED, NAMES.index(name)])
    return tuple({s: int.from_bytes(rng.bytes(32), "little") for s, _ in leaves}
                 for _ in range(MAX_WALKERS))


def starts(name, walkers, scoring="tree"):
    """(walkers, n_leaves, 8): walker w's own start, in the leaf order of the
    program of ``scoring``."""
    prog = program(name, 16, scoring)
    return np.stack([WK.leaf_rows(prog, v) for v in start_values(name)[:walkers]])


consts_of = WK.consts_of


@functools.lru_cache(maxsize=None)
def aims(name):
    """The case's aim table (the leaf order is the same on both layouts)."""
    A = RP.aim_table(trees(name), program(name))
    for a in (A.entries, A.pieces):
        a.setflags(write=False)
    return A


def _record_nodes(name, scoring):
    cs, _, _, T, probes, _ = _built(name)
    atoms = list(T.atom_nodes) if scoring == "tree" else []
    resid = {"tree": list(T.probes), "table": list(probes), "mask": []}[scoring]
    return list(cs), atoms, resid


@functools.lru_cache(maxsize=None)
def _serialized(name, scoring):
    cs, atoms, resid = _record_nodes(name, scoring)
    return evalref.serialize(cs, program(name, 16, scoring), atoms + resid)


def _rows(vals):
    """(n, k, limbs) u64 record values -> (k, 8, n) u32 probe rows."""
    r64 = np.ascontiguousarray(vals[:, :, :4]).view("<u4")
    return np.ascontiguousarray(r64.transpose(1, 2, 0))


def values_fn(name, scoring="tree"):
    """SoA leaves (n_leaves, 8, n) -> (root verdicts (n, n_roots) bool, atom
    verdicts (n, n_atoms) bool, residual values (n_resid, 8, n) u32) from the
    oracle alone; without the atom verdicts for ``table``, the root verdicts
    alone for ``mask``."""
    S, prog = _serialized(name, scoring), program(name, 16, scoring)
    cs, atoms, resid = _record_nodes(name, scoring)
    records = [S.node_index[n.id] for n in cs + atoms + resid]
    n_c, n_a = len(cs), len(atoms)

    def fn(soa):
        _, vals = evalref.run_nodes_soa(S, prog, np.ascontiguousarray(soa), records=records,
                                        chunk=256)
        bits = (vals[:, :n_c, 0] & np.uint64(1)).astype(bool)
        if scoring == "mask":
            return bits
        rows = _rows(vals[:, n_c + n_a:])
        if scoring == "table":
            return bits, rows
        return bits, (vals[:, n_c:n_c + n_a, 0] & np.uint64(1)).astype(bool), rows
    return fn


def _frozen(res):
    for a in (res.leaves, res.trace) + ((res.nfail, res.cost) if hasattr(res, "cost") else ()):
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def reference(name, walkers, lanes, rounds=ROUNDS, scoring="tree", seed=SEED):
    """walk_ref through the oracle from the walkers' starts: ``tree`` with the
    tree scoring, ``aim`` with the aim table besides, ``table`` under the table
    of ``repair.residuals`` on the program that carries its probes."""
    kind = "table" if scoring == "table" else "tree"
    prog = program(name, 16, kind)
    T = trees(name)
    kw = {} if kind == "table" else {"score": RP.tree_scoring(T)}
    if scoring == "aim":
        kw["aims"] = aims(name)
    table = table_scoring(name)[1] if kind == "table" else T.roots
    return _frozen(RP.walk_ref(values_fn(name, kind), default_leafgen(prog), consts_of(prog),
                               starts(name, walkers, kind), table, seed, lanes, rounds, 8, **kw))


@functools.lru_cache(maxsize=None)
def repair_reference(name, lanes, rounds=ROUNDS, seed=SEED):
    """repair_ref through the oracle on the mask-only program from walker 0's
    start."""
    prog = program(name, 16, "mask")
    return _frozen(RP.repair_ref(values_fn(name, "mask"), default_leafgen(prog), consts_of(prog),
                                 starts(name, 1, "mask")[0], seed, lanes, rounds, 8))


@functools.lru_cache(maxsize=None)
def round_inputs(name, walkers, lanes, scoring="tree", seed=SEED):
    """Round 0 of ``reference``: (neighbours (n_leaves, 8, walkers * lanes),
    what ``values_fn`` says of them), walker w in columns w * lanes .."""
    prog = program(name, 16, scoring)
    base = starts(name, walkers, scoring)
    nb = np.concatenate([RP.mutate_ref(default_leafgen(prog), consts_of(prog), base[w],
                                       seed ^ (w * RP.CW & RP.M64), 0, lanes)
                         for w in range(walkers)], axis=2)
    values = values_fn(name, scoring)(nb)
    for a in (nb,) + (values if isinstance(values, tuple) else (values,)):
        a.setflags(write=False)
    return nb, values


@functools.lru_cache(maxsize=None)
def stride_reference(kernel):
    """The strided case under ``kernel``'s seed, through the round of
    STRIDE_SEEDS: (the reference result, the lowest lane of that round's
    minimum key, the number of lanes at that key, the key (nfail, cost)) — the
    key recomputed here from what the oracle said of that round's neighbours
    (the count alone for ``repair``)."""
    seed, rnd, _ = STRIDE_SEEDS[kernel]
    scoring = {"repair": "mask", "walk": "table"}.get(kernel, "tree")
    prog, T = program(STRIDE, 16, scoring), trees(STRIDE)
    fn, seen = values_fn(STRIDE, scoring), []

    def recording(soa):
        seen.append(fn(soa))
        return seen[-1]
    args = (default_leafgen(prog), consts_of(prog))
    start = starts(STRIDE, 1, scoring)
    if kernel == "repair":
        res = RP.repair_ref(recording, *args, start[0], seed, STRIDE_LANES, rnd + 1, 8)
        nfail = (~seen[rnd]).sum(axis=1).astype(np.int64)
        cost = np.zeros_like(nfail)
    elif kernel == "walk":
        table = table_scoring(STRIDE)[1]
        res = RP.walk_ref(recording, *args, start, table, seed, STRIDE_LANES, rnd + 1, 8)
        nfail, cost = RP._score_bits(*seen[rnd], table)
    else:
        kw = {"aims": aims(STRIDE)} if kernel == "walk_aim" else {}
        res = RP.walk_ref(recording, *args, start, T.roots, seed, STRIDE_LANES, rnd + 1, 8,
                          score=RP.tree_scoring(T), **kw)
        nfail, cost = RP.tree_scoring(T)(*seen[rnd])
    key = nfail << 20 | cost
    lane = int(np.argmin(key))
    return _frozen(res), lane, int((key == key[lane]).sum()), (int(nfail[lane]), int(cost[lane]))

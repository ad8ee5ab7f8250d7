"""Test infrastructure of the walk with aims through sums (tests/test_walk_sum.py,
tests/test_gpu_walk_sum.py): the crafted cases, their
eval-form programs with root mask, atom mask, residual probes, side rows and
the arguments' chunks, their tables, the oracle's values as the ``values_fn``
of ``walk_ref``, and the reference runs, computed once per (case, walkers,
lanes, rounds, sync, table, seed).

Every case is in eval form with the default generator and carries the guards
of tests/walk_cases.py on its variables; each start is ``target xor random``.
  sum       a + b = p xor q.  The side p xor q resolves by no rule; a + b is
            linear with the targets a and b (two XOR-mode entries, both +,
            one side row).  The start's b is (p xor q) - a with 200 random
            bits flipped
  spend     bvult(K, bal - v) and bvule(bal - v, t + 3), t = p xor q; K is a
            numeral whose 100 top bits are a random pattern P, and two more
            roots pin those bits of p to P and of q to zeros, as `hash` of
            tests/uf_cases.py pins them to ones (with all ones the window
            K .. t + 3 ends just below 2^256, and a copy of v to bal with one
            more bit flipped lands 0 - 2^154 in it: the walk of §3.14 closed
            that case in round 1); the halves of bal are exchanged as those
            of f(w) are there, so that a copy of p to bal does not land in
            the window; and each pin is ten roots of ten bits, so that a move
            which widens the window by overwriting p breaks ten roots, not
            one (with one root per pin round 0, which has no aim yet, adopted
            such a move at a lower cost than the start's, and neither walk
            left it).  K is a numeral and t + 3 a sum whose one term
            resolves by no rule, so of the orders' sides bal - v alone gives
            entries: bal (+, two pieces) and v (-) HIGH_STRICT for root 0 and
            LOW for root 1, after the twenty XOR entries of p and q.  The start has p and q
            right and bal - v = (t + 1) xor random, below K
  opaque    bvmul(y, z) - x = p xor q: the term y * z resolves by no rule and
            need not; the one target is x, with sign -.  The start's x is
            y * z - (p xor q) with 200 random bits flipped
  selector  bvand(0xffffffff, bvudiv(w, 2^224)) = 0xa9059cbb, the dispatcher's
            selector word: the mask and shift rules alone resolve the side to
            bits 224 .. 255 of w, a plain XOR entry; no linear entry, no side
            row.  The start's selector is the target xor 32 random bits
`caps` is generated, not crafted: 64 roots a_i + b_i = K_i over 64-bit
variables, which gives 64 side rows and 128 linear entries.

Chosen max_rounds and what was observed (one walker, 4096 lanes, seed SEED;
tests/test_walk_sum.py asserts (a) no model among the generator's lanes x
max_rounds candidates, (b) walk_ref with the tables of §3.14 is still failing
after max_rounds, (c) with the tables of §3.15 it reaches nfail == 0 within
half of max_rounds; for `selector` that the new table closes it in round 1 and
the old one in a later round or not at all):
  sum       max_rounds %d: the first round with nfail == 0 is round %d
  spend     max_rounds %d: round %d
  opaque    max_rounds %d: round %d
  selector  max_rounds %d: round %d (the table of §3.14: round %d)
"""

import functools

import numpy as np

import tree_cases as TC
import uf_cases as UC
import walk_cases as WK
from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import default_leafgen
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N
from oracle import evalref

SEED = TC.SEED
LANES = 4096
NAMES = ("sum", "spend", "opaque", "selector")
STUCK = ("sum", "spend", "opaque")                 # the table of §3.14 does not close them
MAX_ROUNDS = {"sum": 16, "spend": 16, "opaque": 16, "selector": 32, "caps": 4}
FIRST_ZERO = {"sum": 1, "spend": 1, "opaque": 1, "selector": 1}    # observed (see above)
SELECTOR_OLD = 5                                   # observed: `selector` under §3.14's table
__doc__ = __doc__ % (tuple(v for n in NAMES for v in (MAX_ROUNDS[n], FIRST_ZERO[n])) +
                     (SELECTOR_OLD,))

_rng = np.random.default_rng(0x73756D)
_R = [int.from_bytes(_rng.bytes(32), "little") for _ in range(16)]
M256 = (1 << 256) - 1
AT = (64, 128)
SELECTOR = 0xa9059cbb
N_CAPS = 64


def _case(name):
    """(constraints, start {variable: value})."""
    var = lambda s, w=256: N.bv_var(s, w)
    op, num = N.bv_op, lambda v, w=256: N.bv_num(v, w)
    g = lambda v: WK._guarded(v, AT)
    if name == "sum":
        a, b, p, q = (var(c) for c in "abpq")
        cs = [N.eq(op("bvadd", a, b), op("bvxor", p, q))]
        for v in (a, b, p, q):
            cs += WK._guards(v, AT)
        av, pv, qv = g(_R[0]), g(_R[1]), g(_R[2]) ^ (0x1111 << 64 | 0x1111 << 128)
        bv = g(((pv ^ qv) - av & M256) ^ _R[3] >> 56)
        return cs, {"a": av, "b": bv, "p": pv, "q": qv}
    if name == "spend":
        bal, v, p, q = var("bal"), var("v"), var("p"), var("q")
        ones = _R[12] >> 156 | 1 << 98                               # a pattern, not all ones
        K = ones << 156 | _R[0] >> 120
        left, t = op("bvsub", UC._swap(bal), v), op("bvxor", p, q)
        cs = [N.bv_cmp("bvult", num(K), left),
              N.bv_cmp("bvule", left, op("bvadd", t, num(3)))]
        for lo in range(156, 256, 10):                   # ten roots per pin: see above
            cs += [N.eq(N.extract(lo + 9, lo, p), num(ones >> (lo - 156) & 0x3FF, 10)),
                   N.eq(N.extract(lo + 9, lo, q), num(0, 10))]
        for x in (bal, v, p, q):
            cs += WK._guards(x, AT)
        low = (1 << 156) - 1
        pv = ones << 156 | g(_R[2]) & low
        qv = (g(_R[1]) ^ (0x1111 << 64 | 0x1111 << 128)) & low
        tv = pv ^ qv
        sv = (tv + 1) ^ _R[3]                                        # target xor random
        vv = g(_R[4])
        balv = (sv + vv) & M256
        balv = (balv << 128 | balv >> 128) & M256
        assert K < tv and sv < K
        assert all((balv >> lo & 0xFFFF) not in (0, 0xFFFF) for lo in AT)
        return cs, {"bal": balv, "v": vv, "p": pv, "q": qv}
    if name == "opaque":
        x, y, z, p, q = (var(c) for c in "xyzpq")
        cs = [N.eq(op("bvsub", op("bvmul", y, z), x), op("bvxor", p, q))]
        for v in (x, y, z, p, q):
            cs += WK._guards(v, AT)
        yv, zv, pv = g(_R[5]), g(_R[6]), g(_R[7])
        qv = g(_R[8]) ^ (0x1111 << 64 | 0x1111 << 128)
        xv = g((yv * zv - (pv ^ qv) & M256) ^ _R[9] >> 56)
        return cs, {"x": xv, "y": yv, "z": zv, "p": pv, "q": qv}
    if name == "selector":
        w = var("w")
        word = op("bvand", num(0xffffffff), op("bvudiv", w, num(1 << 224)))
        cs = [N.eq(word, num(SELECTOR))] + WK._guards(w, AT)
        wv = g(_R[10]) & ((1 << 224) - 1) | (SELECTOR ^ _R[11] & 0xffffffff) << 224
        return cs, {"w": wv}
    if name == "caps":
        cs, start = [], {}
        rng = np.random.default_rng(0x63617073)
        for i in range(N_CAPS):
            a, b = var("a%02d" % i, 64), var("b%02d" % i, 64)
            cs.append(N.eq(op("bvadd", a, b), num(int(rng.integers(1, 1 << 62)), 64)))
            start["a%02d" % i] = int(rng.integers(1, 1 << 62))
            start["b%02d" % i] = int(rng.integers(1, 1 << 62))
        return cs, start
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _built(name):
    """The case's nodes, built in one order inside a scope of their own (a
    program's schedule follows the node ids)."""
    with N.fresh_scope():
        cs, start = _case(name)
        trees = RP.distance_trees(cs)
        mask = CS.mask_probes(cs)
        amask = CS.mask_probes(trees.atom_nodes)
        sprobes = RP.sum_probes(trees)
        apps, uprobes = RP.uf_probes(trees)
    for a in (trees.roots, trees.atoms, trees.code):
        a.setflags(write=False)
    return cs, start, mask, amask, trees, tuple(apps), tuple(uprobes), tuple(sprobes)


def case(name):
    """(constraints, start assignment {variable: value})."""
    return _built(name)[:2]


def trees(name):
    return _built(name)[4]


def apps(name):
    return _built(name)[5]


def sprobes(name):
    return _built(name)[7]


@functools.lru_cache(maxsize=None)
def program(name, nreg=16):
    """The case's eval-form program: root mask, atom mask, the trees'
    residuals, the side rows, the arguments' chunks."""
    cs, _, mask, amask, T, _, up, sp = _built(name)
    return compile_constraints(cs, mask + amask + list(T.probes) + list(sp) + list(up), nreg=nreg)


@functools.lru_cache(maxsize=None)
def tables(name):
    """(Bounds, Ufs, Sums) of §3.15, built outside the scope the nodes were
    built in."""
    B, U, S = RP.sum_table(case(name)[0], trees(name), program(name), apps(name))
    for a in (B.entries, B.pieces, B.fixed, U.slots, U.funcs, U.cands, U.ukeys, S.lin):
        a.setflags(write=False)
    return B, U, S


@functools.lru_cache(maxsize=None)
def old_tables(name):
    """(Bounds, Ufs) of §3.14 on the same program."""
    return RP.uf_table(case(name)[0], trees(name), program(name), apps(name))


def n_before(name):
    """The probes in front of the U rows."""
    _, _, mask, amask, T, _, _, sp = _built(name)
    return len(mask) + len(amask) + len(T.probes) + len(sp)


def view(name, nreg=16):
    """What the walk loads: the program up to its U rows (``repair.uf_view``)."""
    U = tables(name)[1]
    return RP.uf_view(program(name, nreg), n_before(name) + U.n_arg_rows, U.keep)


leaf_rows = WK.leaf_rows


def start_rows(name):
    return leaf_rows(program(name), case(name)[1])


def starts(name, walkers):
    """(walkers, n_leaves, 8): the case's start for every walker."""
    return np.repeat(start_rows(name)[None], walkers, axis=0)


consts_of = WK.consts_of


@functools.lru_cache(maxsize=None)
def _serialized(name):
    cs, _, _, _, T, _, up, sp = _built(name)
    return evalref.serialize(cs, program(name),
                             list(T.atom_nodes) + list(T.probes) + list(sp) + list(up))


def values_fn(name, srows=True):
    """SoA leaves (n_leaves, 8, n) -> (root verdicts (n, n_roots) bool, atom
    verdicts (n, n_atoms) bool, residual values (n_resid, 8, n) u32, U rows
    (n_urows, 8, n) u32, side rows (n_srows, 8, n) u32), from the oracle alone.
    ``srows`` False: the first four, what ``walk_ref(ufs=)`` takes."""
    S, prog = _serialized(name), program(name)
    cs, _, _, _, T, _, up, sp = _built(name)
    nodes = list(cs) + list(T.atom_nodes) + list(T.probes) + list(sp) + list(up)
    records = [S.node_index[n.id] for n in nodes]
    n_c, n_a, n_r, n_s = len(cs), len(T.atom_nodes), len(T.probes), len(sp)

    def fn(soa):
        _, vals = evalref.run_nodes_soa(S, prog, np.ascontiguousarray(soa), records=records,
                                        chunk=256)
        bits = (vals[:, :n_c, 0] & np.uint64(1)).astype(bool)
        abits = (vals[:, n_c:n_c + n_a, 0] & np.uint64(1)).astype(bool)
        at = n_c + n_a + n_r
        out = (bits, abits, TC._rows(vals[:, n_c + n_a:at]), TC._rows(vals[:, at + n_s:]))
        return out + (TC._rows(vals[:, at:at + n_s]),) if srows else out
    return fn


@functools.lru_cache(maxsize=None)
def reference(name, walkers=1, lanes=LANES, max_rounds=None, sync_every=8, sums=True, seed=SEED):
    """walk_ref with the tree scoring through the oracle from the case's
    start; ``sums``: with the case's tables of §3.15, else with those of
    §3.14."""
    prog = program(name)
    T = trees(name)
    if sums:
        B, U, S = tables(name)
        kw = dict(bounds=B, ufs=U, sums=S)
    else:
        B, U = old_tables(name)
        kw = dict(bounds=B, ufs=U)
    res = RP.walk_ref(values_fn(name, sums), default_leafgen(prog), consts_of(prog),
                      starts(name, walkers), T.roots, seed, lanes,
                      MAX_ROUNDS[name] if max_rounds is None else max_rounds, sync_every,
                      score=RP.tree_scoring(T), **kw)
    for a in (res.leaves, res.nfail, res.cost, res.trace):
        a.setflags(write=False)
    return res


def generator_hits(name, n):
    """Satisfying candidates among the default generator's first n."""
    cs = case(name)[0]
    prog = compile_constraints(cs, _built(name)[2], nreg=16)
    bits = evalref.run_gen(evalref.serialize(cs, prog), prog, SEED, 0, 0, n, per_root=True)
    return int(bits.all(axis=1).sum())


def first_zero(res):
    """The first round whose best neighbour fails no root, or None."""
    hit = np.flatnonzero(res.trace[0, :res.rounds, 0] == 0)
    return int(hit[0]) if len(hit) else None

"""Test infrastructure of the tree-scored walk (tests/test_walk_tree.py,
tests/test_gpu_walk_tree.py): the crafted cases, their
eval-form programs with root mask, atom mask and residual probes, the oracle's
verdicts, atom verdicts and residual values as the ``values_fn`` of
``walk_ref``, and the reference runs, computed once per (case, walkers, lanes,
rounds, sync).

Every case is in eval form with the default generator and carries the guards
of tests/walk_cases.py.  Each is one root short of a model, many moves away,
and that root is FLAT under ``repair.residuals``:
  chain  not (select(store(K(256 -> 8, 0), h, v), arg) = 0): arg the concat of
         32 one-byte leaves, h a 256-bit leaf with guards, v an 8-bit leaf —
         a negated equality over a store-chain read whose only hit needs
         arg = h (and v != 0).  Tree: AND(HAMMING(h = arg), FLAT(v != 0)).
         The start has arg about half of the 256 bits from h, and v = 0
  conj   ONE root and(x ^ y = z, not (q - p <= LO), q - p < HI): x, y, z
         256-bit, p, q 64-bit, guards on x, y, z and p.  Tree: AND(HAMMING,
         MAGNITUDE, MAGNITUDE).  The start has x ^ y about 128 bits from z
         and q - p = 2^40 + 1
  nest   ONE root and(a512 = concat(u, w), or(and(K <= h, h < K', h urem 64 =
         0), and(h = H, false))): a512 the concat of a 128-, a 256- and a
         128-bit leaf, so the 512-bit equality becomes two 256-bit chunks
         whose extracts cut through a leaf; the second arm is infinitely far
         and folds away.  Tree: AND(HAMMING, HAMMING, MAGNITUDE, MAGNITUDE,
         HAMMING).  The start has about 64 bits of a512 wrong and h random

Chosen max_rounds and what was observed (one walker, 4096 lanes, seed SEED;
tests/test_walk_tree.py asserts (a) no model among the generator's lanes x
max_rounds candidates, (b) walk_ref under the residuals() table is still
failing after max_rounds, (c) the tree walk reaches nfail == 0 within half of
max_rounds):
  chain  max_rounds %d: the tree walk's first round with nfail == 0 is round %d
  conj   max_rounds %d: round %d
  nest   max_rounds %d: round %d
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

SEED = 0x74726565
LANES = 4096
NAMES = ("chain", "conj", "nest")
MAX_ROUNDS = {"chain": 128, "conj": 128, "nest": 96}
FIRST_ZERO = {"chain": 44, "conj": 53, "nest": 36}              # observed (see above)
__doc__ = __doc__ % tuple(v for n in NAMES for v in (MAX_ROUNDS[n], FIRST_ZERO[n]))

_rng = np.random.default_rng(0x74726565)
_R = [int.from_bytes(_rng.bytes(32), "little") for _ in range(12)]
LO, HI = WK.LO, WK.HI
M64 = (1 << 64) - 1
M256 = (1 << 256) - 1
# the window of `nest`: none of K - 1, K, K + 1 (the generator's pool values) is
# a multiple of 64, and K = 62 (mod 64): the aligned K + 2 is one STEP move from
# K and from K + 1.  (With K = 2 (mod 64) the strict-improvement rule has a
# local minimum at h = K, one bit from aligned: every single move that aligns
# h leaves the window — the plateau that DESIGN.md §3.11 leaves unbuilt.)
K_LO = _R[8] & ~63 | 62
K_HI = K_LO + (1 << 20)
H_FAR = _R[9]


def _case(name):
    if name == "chain":
        h, v = N.bv_var("h", 256), N.bv_var("v", 8)
        arg = N.concat(*[N.bv_var("b%02d" % i, 8) for i in reversed(range(32))])
        read = N.select(N.store(N.const_array(256, N.bv_num(0, 8)), h, v), arg)
        cs = [N.bool_op("not", N.eq(read, N.bv_num(0, 8)))] + WK._guards(h, (64, 128))
        hv = WK._guarded(_R[0], (64, 128))
        av = hv ^ _R[1]                                   # about 128 bits away
        start = {"h": hv, "v": 0}
        start.update({"b%02d" % i: av >> (8 * i) & 0xFF for i in range(32)})
        return cs, start
    if name == "conj":
        x, y, z = (N.bv_var(s, 256) for s in "xyz")
        p, q = N.bv_var("p", 64), N.bv_var("q", 64)
        d = N.bv_op("bvsub", q, p)
        cs = [N.bool_op("and", N.eq(N.bv_op("bvxor", x, y), z),
                        N.bool_op("not", N.bv_cmp("bvule", d, N.bv_num(LO, 64))),
                        N.bv_cmp("bvult", d, N.bv_num(HI, 64)))]
        for t in (x, y, z):
            cs += WK._guards(t, (64, 128))
        cs += WK._guards(p, (16, 40))
        pv = WK._guarded(_R[5] & M64, (16, 40))
        start = {s: WK._guarded(r, (64, 128)) for s, r in zip("xyz", _R[2:5])}
        start.update(p=pv, q=(pv + (1 << 40) + 1) & M64)
        return cs, start
    if name == "nest":
        hi, mid, lo = N.bv_var("a_hi", 128), N.bv_var("a_mid", 256), N.bv_var("a_lo", 128)
        u, w, h = N.bv_var("u", 256), N.bv_var("w", 256), N.bv_var("h", 256)
        num = lambda v: N.bv_num(v, 256)
        near = N.bool_op("and", N.bv_cmp("bvule", num(K_LO), h), N.bv_cmp("bvult", h, num(K_HI)),
                         N.eq(N.bv_op("bvurem", h, num(64)), num(0)))
        far = N.bool_op("and", N.eq(h, num(H_FAR)), N.bool_val(False))
        cs = [N.bool_op("and", N.eq(N.concat(hi, mid, lo), N.concat(u, w)),
                        N.bool_op("or", near, far))]
        for t in (u, w, h):
            cs += WK._guards(t, (64, 128))
        uv, wv = WK._guarded(_R[6], (64, 128)), WK._guarded(_R[7], (64, 128))
        wrong = int.from_bytes(_rng.bytes(64), "little") & int.from_bytes(_rng.bytes(64), "little") \
            & int.from_bytes(_rng.bytes(64), "little")    # about 64 of the 512 bits
        a = (uv << 256 | wv) ^ wrong
        return cs, {"a_hi": a >> 384, "a_mid": a >> 128 & M256, "a_lo": a & ((1 << 128) - 1),
                    "u": uv, "w": wv, "h": WK._guarded(_R[10], (64, 128))}
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _built(name):
    """The case's nodes, built in one order inside a scope of their own (a
    program's schedule follows the node ids)."""
    with N.fresh_scope():
        cs, start = _case(name)
        trees = RP.distance_trees(cs)
        probes, table = RP.residuals(cs)
        mask = CS.mask_probes(cs)
        amask = CS.mask_probes(trees.atom_nodes)
    for a in (trees.roots, trees.atoms, trees.code, table):
        a.setflags(write=False)
    return cs, start, mask, amask, trees, tuple(probes), table


def case(name):
    """(constraints, start assignment {symbol: value})."""
    return _built(name)[:2]


def trees(name):
    return _built(name)[4]


def table_scoring(name):
    """(residual probe nodes, table) of ``repair.residuals``: today's table."""
    return _built(name)[5:]


@functools.lru_cache(maxsize=None)
def program(name, nreg=16, scoring="tree"):
    """The case's eval-form program: root mask, then (``tree``) atom mask and
    the trees' residuals, or (``table``) the residuals of today's table."""
    cs, _, mask, amask, T, probes, _ = _built(name)
    extra = amask + list(T.probes) if scoring == "tree" else list(probes)
    return compile_constraints(cs, mask + extra, nreg=nreg)


def start_rows(name, scoring="tree"):
    return WK.leaf_rows(program(name, 16, scoring), case(name)[1])


def starts(name, walkers):
    """(walkers, n_leaves, 8): the case's start for every walker."""
    return np.repeat(start_rows(name)[None], walkers, axis=0)


consts_of = WK.consts_of


@functools.lru_cache(maxsize=None)
def _serialized(name, scoring="tree"):
    cs, _, _, _, T, probes, _ = _built(name)
    extra = list(T.atom_nodes) + list(T.probes) if scoring == "tree" else list(probes)
    return evalref.serialize(cs, program(name, 16, scoring), extra)


def _rows(vals):
    """(n, k, limbs) u64 record values -> (k, 8, n) u32 probe rows."""
    r64 = np.ascontiguousarray(vals[:, :, :4]).view("<u4")
    return np.ascontiguousarray(r64.transpose(1, 2, 0))


def values_fn(name, scoring="tree"):
    """SoA leaves (n_leaves, 8, n) -> (root verdicts (n, n_roots) bool, atom
    verdicts (n, n_atoms) bool, residual values (n_resid, 8, n) u32) — without
    the atom verdicts for ``table`` — from the oracle alone."""
    S, prog = _serialized(name, scoring), program(name, 16, scoring)
    cs, _, _, _, T, probes, _ = _built(name)
    atoms = list(T.atom_nodes) if scoring == "tree" else []
    resid = list(T.probes) if scoring == "tree" else list(probes)
    records = [S.node_index[n.id] for n in list(cs) + atoms + resid]
    n_c, n_a = len(cs), len(atoms)

    def fn(soa):
        _, vals = evalref.run_nodes_soa(S, prog, np.ascontiguousarray(soa), records=records,
                                        chunk=256)
        bits = (vals[:, :n_c, 0] & np.uint64(1)).astype(bool)
        abits = (vals[:, n_c:n_c + n_a, 0] & np.uint64(1)).astype(bool)
        rows = _rows(vals[:, n_c + n_a:])
        return (bits, abits, rows) if scoring == "tree" else (bits, rows)
    return fn


def bits_fn(name):
    fn = values_fn(name)
    return lambda soa: fn(soa)[0]


@functools.lru_cache(maxsize=None)
def reference(name, walkers=1, lanes=LANES, max_rounds=None, sync_every=8):
    """walk_ref with the tree scoring through the oracle from the case's start."""
    prog = program(name)
    T = trees(name)
    res = RP.walk_ref(values_fn(name), default_leafgen(prog), consts_of(prog), starts(name, walkers),
                      T.roots, SEED, lanes, MAX_ROUNDS[name] if max_rounds is None else max_rounds,
                      sync_every, score=RP.tree_scoring(T))
    for a in (res.leaves, res.nfail, res.cost, res.trace):
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def table_reference(name):
    """walk_ref under today's residuals() table from the same start, same
    budget."""
    prog = program(name, 16, "table")
    return RP.walk_ref(values_fn(name, "table"), default_leafgen(prog), consts_of(prog),
                       start_rows(name, "table")[None], table_scoring(name)[1], SEED, LANES,
                       MAX_ROUNDS[name], 8)


def generator_hits(name, n):
    """Satisfying candidates among the default generator's first n."""
    cs = case(name)[0]
    prog = compile_constraints(cs, _built(name)[2], nreg=16)
    bits = evalref.run_gen(evalref.serialize(cs, prog), prog, SEED, 0, 0, n, per_root=True)
    return int(bits.all(axis=1).sum())

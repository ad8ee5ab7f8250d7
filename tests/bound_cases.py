"""Test infrastructure of the walk with aims for orders
(tests/test_walk_bound.py, tests/test_gpu_walk_bound.py): the
crafted cases, their eval-form programs with root mask, atom mask and residual
probes, their tables, the oracle's values as the ``values_fn`` of
``walk_ref``, and the reference runs, computed once per (case, walkers, lanes,
rounds, sync, moves, seed).

Every case is in eval form with the default generator and carries the guards
of tests/walk_cases.py.  Each asks for a value inside a narrow window whose
edge is another term's value; one side of both orders is made of leaves and
starts about 128 bits away (``target xor random``).  A MAGNITUDE distance is 1
+ bitlen(lo - hi): the plain moves follow it about one bit per round when the
value is spread over small leaves.
  window  bvule(h, arg) and bvule(arg, h + 3): arg the concat of 32 one-byte
          leaves, h a guarded 256-bit leaf whose top bit is clear at the start.
          Entries: h (LOW) and arg (HIGH) of the first order, arg (LOW) of the
          second (h + 3 does not resolve)
  signed  bvslt(t, d) and not bvsgt(d, t + 2): d = concat(p, q, s) of 100, 13
          and 143 bits (no piece edge on a multiple of 32, carries across
          limbs), t = x xor y xor z, guarded; the second root is a negated
          order, converted to bvsle(d, t + 2).  Entries: d HIGH_STRICT, d LOW
  fixed   bvult(t, v) and bvule(v, t + 0x200): v = concat(31 one-byte leaves,
          the numeral 0x80), t = x xor y.  The fixed bits sit below the
          pieces: a gather without them takes another target.  Entries: v
          HIGH_STRICT, v LOW.  Round 1's aimed lane leaves (1 failing, cost 8):
          the numeral byte keeps v below t

Chosen max_rounds and what was observed (one walker, 4096 lanes, seed SEED;
tests/test_walk_bound.py asserts (a) no model among the generator's lanes x
max_rounds candidates, (b) walk_ref with the tree scoring and the aim table
of §3.12 is still failing after max_rounds, (c) with the table of §3.13 it
reaches nfail == 0 within half of max_rounds):
  window  max_rounds %d: the first round with nfail == 0 is round %d
  signed  max_rounds %d: round %d
  fixed   max_rounds %d: round %d
"""

import functools

import numpy as np

import tree_cases as TC
import walk_cases as WK
from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import default_leafgen
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N
from oracle import evalref

SEED = TC.SEED
LANES = 4096
NAMES = ("window", "signed", "fixed")
MAX_ROUNDS = {"window": 96, "signed": 32, "fixed": 64}
FIRST_ZERO = {"window": 1, "signed": 1, "fixed": 2}             # observed (see above)
__doc__ = __doc__ % tuple(v for n in NAMES for v in (MAX_ROUNDS[n], FIRST_ZERO[n]))

_rng = np.random.default_rng(0x626F756E64)
_R = [int.from_bytes(_rng.bytes(32), "little") for _ in range(8)]
M256 = (1 << 256) - 1
AT = (64, 128)


def _case(name):
    num = lambda v: N.bv_num(v, 256)
    if name == "window":
        h = N.bv_var("h", 256)
        arg = N.concat(*[N.bv_var("b%02d" % i, 8) for i in reversed(range(32))])
        cs = [N.bv_cmp("bvule", h, arg), N.bv_cmp("bvule", arg, N.bv_op("bvadd", h, num(3)))]
        cs += WK._guards(h, AT)
        hv = WK._guarded(_R[0], AT) & (M256 >> 1)
        av = hv ^ _R[1]
        start = {"b%02d" % i: av >> (8 * i) & 0xFF for i in range(32)}
        start["h"] = hv
        return cs, start
    if name == "signed":
        p, q, s = N.bv_var("p", 100), N.bv_var("q", 13), N.bv_var("s", 143)
        x, y, z = N.bv_var("x", 256), N.bv_var("y", 256), N.bv_var("z", 256)
        d, t = N.concat(p, q, s), N.bv_op("bvxor", x, y, z)
        cs = [N.bv_cmp("bvslt", t, d),
              N.bool_op("not", N.bv_cmp("bvsgt", d, N.bv_op("bvadd", t, num(2))))]
        for v in (x, y, z):
            cs += WK._guards(v, AT)
        xv, yv, zv = (WK._guarded(r, AT) for r in (_R[2], _R[3], _R[4]))
        dv = xv ^ yv ^ zv ^ _R[5]
        return cs, {"p": dv >> 156, "q": dv >> 143 & 0x1FFF, "s": dv & ((1 << 143) - 1),
                    "x": xv, "y": yv, "z": zv}
    if name == "fixed":
        x, y = N.bv_var("x", 256), N.bv_var("y", 256)
        v = N.concat(*([N.bv_var("b%02d" % i, 8) for i in reversed(range(1, 32))]
                       + [N.bv_num(0x80, 8)]))
        t = N.bv_op("bvxor", x, y)
        cs = [N.bv_cmp("bvult", t, v), N.bv_cmp("bvule", v, N.bv_op("bvadd", t, num(0x200)))]
        for u in (x, y):
            cs += WK._guards(u, AT)
        xv, yv = WK._guarded(_R[6], AT), WK._guarded(_R[7], AT)
        # the low byte of t + 1 above the numeral: the aimed v = t + 1 with its
        # low byte 0x80 is then 0x43 below t, and one more step of 0x100 away
        xv = xv & ~0xFF | (yv & 0xFF) ^ 0xC3
        vv = xv ^ yv ^ _R[1]
        start = {"b%02d" % i: vv >> (8 * i) & 0xFF for i in range(1, 32)}
        start.update(x=xv, y=yv)
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
    for a in (trees.roots, trees.atoms, trees.code):
        a.setflags(write=False)
    return cs, start, mask, amask, trees


def case(name):
    """(constraints, start assignment {symbol: value})."""
    return _built(name)[:2]


def trees(name):
    return _built(name)[4]


@functools.lru_cache(maxsize=None)
def program(name, nreg=16):
    """The case's eval-form program: root mask, atom mask, the trees' residuals."""
    cs, _, mask, amask, T = _built(name)
    return compile_constraints(cs, mask + amask + list(T.probes), nreg=nreg)


@functools.lru_cache(maxsize=None)
def aims(name):
    """The case's aim table of §3.12 (no order entry)."""
    return RP.aim_table(trees(name), program(name))


@functools.lru_cache(maxsize=None)
def bounds(name):
    """The case's table, built outside the scope its nodes were built in (the
    leaf order of a case is the same on both register layouts)."""
    B = RP.bound_table(case(name)[0], trees(name), program(name))
    for a in (B.entries, B.pieces, B.fixed):
        a.setflags(write=False)
    return B


def start_rows(name):
    return WK.leaf_rows(program(name), case(name)[1])


def starts(name, walkers):
    """(walkers, n_leaves, 8): the case's start for every walker."""
    return np.repeat(start_rows(name)[None], walkers, axis=0)


consts_of = WK.consts_of


@functools.lru_cache(maxsize=None)
def _serialized(name):
    cs, _, _, _, T = _built(name)
    return evalref.serialize(cs, program(name), list(T.atom_nodes) + list(T.probes))


def values_fn(name):
    """SoA leaves (n_leaves, 8, n) -> (root verdicts (n, n_roots) bool, atom
    verdicts (n, n_atoms) bool, residual values (n_resid, 8, n) u32), from the
    oracle alone."""
    S, prog = _serialized(name), program(name)
    cs, _, _, _, T = _built(name)
    records = [S.node_index[n.id] for n in list(cs) + list(T.atom_nodes) + list(T.probes)]
    n_c, n_a = len(cs), len(T.atom_nodes)

    def fn(soa):
        _, vals = evalref.run_nodes_soa(S, prog, np.ascontiguousarray(soa), records=records,
                                        chunk=256)
        bits = (vals[:, :n_c, 0] & np.uint64(1)).astype(bool)
        abits = (vals[:, n_c:n_c + n_a, 0] & np.uint64(1)).astype(bool)
        return bits, abits, TC._rows(vals[:, n_c + n_a:])
    return fn


@functools.lru_cache(maxsize=None)
def reference(name, walkers=1, lanes=LANES, max_rounds=None, sync_every=8, bound=True, seed=SEED):
    """walk_ref with the tree scoring through the oracle from the case's
    start; ``bound``: with the case's table, else with the aim table of §3.12."""
    prog = program(name)
    T = trees(name)
    kw = dict(bounds=bounds(name)) if bound else dict(aims=aims(name))
    res = RP.walk_ref(values_fn(name), default_leafgen(prog), consts_of(prog), starts(name, walkers),
                      T.roots, seed, lanes, MAX_ROUNDS[name] if max_rounds is None else max_rounds,
                      sync_every, score=RP.tree_scoring(T), **kw)
    for a in (res.leaves, res.nfail, res.cost, res.trace):
        a.setflags(write=False)
    return res


def generator_hits(name, n):
    """Satisfying candidates among the default generator's first n."""
    cs = case(name)[0]
    prog = compile_constraints(cs, _built(name)[2], nreg=16)
    bits = evalref.run_gen(evalref.serialize(cs, prog), prog, SEED, 0, 0, n, per_root=True)
    return int(bits.all(axis=1).sum())

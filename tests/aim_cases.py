"""Test infrastructure of the aimed walk (tests/test_walk_aim.py,
tests/test_gpu_walk_aim.py): the crafted cases, their
eval-form programs with root mask, atom mask and residual probes, their aim
tables, the oracle's values as the ``values_fn`` of ``walk_ref``, and the
reference runs, computed once per (case, walkers, lanes, rounds, sync, aims).

Every case is in eval form with the default generator and carries the guards
of tests/walk_cases.py.  Each has a positive equality whose one side is made
of leaves, many bits away, and a COUPLING root over a block of 24 of those
bits, ``or(extract(block, a xor b) = 0xFFFFFF, extract(block, a xor b) = 0)``:
the start has the block's bits all wrong, so the coupling root holds, every
move that corrects some but not all of them breaks it, and (failing roots,
cost) never improves by single-leaf moves.  The aimed move flips all of them
at once.
  bytes  the `chain` case of tests/tree_cases.py (arg the concat of 32
         one-byte leaves, h a 256-bit leaf) and the coupling root over bits
         0..23 of arg xor h: three byte leaves.  Entries: h (one piece) and
         arg (32 pieces)
  wide   the `nest` case: the 512-bit equality concat(a_hi, a_mid, a_lo) =
         concat(u, w) becomes two 256-bit chunks that cut a_mid at bit 128
         (pieces with leaf_bit 128), and the coupling root over bits 52..75
         of a_mid xor its target, across the limb boundary at 64.  Entries:
         both sides of both chunks
  odd    ONE simple root concat(p, q, s) = x xor y xor z with p, q, s of 100,
         13 and 143 bits (no piece edge on a multiple of 32), guards on x, y
         and z, and the coupling root over bits 138..161: all three leaves.
         One entry (the other side does not resolve).  Three words, and no
         numeral: the generator's candidates have guarded leaves near one
         another and p, q, s near its pool values, so x xor y alone is a few
         pool moves from a generated p, q, s, and the pieces of a numeral
         would be in the pool

Chosen max_rounds and what was observed (one walker, 4096 lanes, seed SEED;
tests/test_walk_aim.py asserts (a) no model among the generator's lanes x
max_rounds candidates, (b) walk_ref with the tree scoring and no aims is still
failing after max_rounds, (c) with aims it reaches nfail == 0 within half of
max_rounds):
  bytes  max_rounds %d: the aimed walk's first round with nfail == 0 is round %d
  wide   max_rounds %d: round %d
  odd    max_rounds %d: round %d
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
NAMES = ("bytes", "wide", "odd")
MAX_ROUNDS = {"bytes": 96, "wide": 96, "odd": 64}
FIRST_ZERO = {"bytes": 2, "wide": 11, "odd": 1}                 # observed (see above)
__doc__ = __doc__ % tuple(v for n in NAMES for v in (MAX_ROUNDS[n], FIRST_ZERO[n]))

_rng = np.random.default_rng(0x61696D)
_R = [int.from_bytes(_rng.bytes(32), "little") for _ in range(4)]
M256 = (1 << 256) - 1
BLOCK = 24
_wide_rng = np.random.default_rng(0x77696465)
_WIDE_WRONG = int.from_bytes(_wide_rng.bytes(64), "little") & int.from_bytes(
    _wide_rng.bytes(64), "little") & int.from_bytes(_wide_rng.bytes(64), "little")


def _coupling(diff, lo):
    """Bits lo .. lo + 23 of ``diff`` are all ones or all zeros."""
    blk = N.extract(lo + BLOCK - 1, lo, diff)
    return N.bool_op("or", N.eq(blk, N.bv_num((1 << BLOCK) - 1, BLOCK)),
                     N.eq(blk, N.bv_num(0, BLOCK)))


def _all_wrong(v, target, lo):
    """``v`` with bits lo .. lo + 23 the complement of ``target``'s."""
    m = ((1 << BLOCK) - 1) << lo
    return v & ~m | ~target & m


def _case(name):
    if name == "bytes":
        cs, start = TC._case("chain")
        h = N.bv_var("h", 256)
        arg = N.concat(*[N.bv_var("b%02d" % i, 8) for i in reversed(range(32))])
        cs = cs + [_coupling(N.bv_op("bvxor", arg, h), 0)]
        av = sum(start["b%02d" % i] << (8 * i) for i in range(32))
        av = _all_wrong(av, start["h"], 0)
        start = dict(start)
        start.update({"b%02d" % i: av >> (8 * i) & 0xFF for i in range(32)})
        return cs, start
    if name == "wide":
        # the `nest` case built here, not through tree_cases._case: that one
        # draws its wrong bits from tree_cases' own generator, and a second
        # draw would change what tests/tree_cases.py builds afterwards
        hi, mid, lo = N.bv_var("a_hi", 128), N.bv_var("a_mid", 256), N.bv_var("a_lo", 128)
        u, w, h = N.bv_var("u", 256), N.bv_var("w", 256), N.bv_var("h", 256)
        num = lambda v: N.bv_num(v, 256)
        near = N.bool_op("and", N.bv_cmp("bvule", num(TC.K_LO), h),
                         N.bv_cmp("bvult", h, num(TC.K_HI)),
                         N.eq(N.bv_op("bvurem", h, num(64)), num(0)))
        far = N.bool_op("and", N.eq(h, num(TC.H_FAR)), N.bool_val(False))
        target = N.concat(N.extract(127, 0, u), N.extract(255, 128, w))
        cs = [N.bool_op("and", N.eq(N.concat(hi, mid, lo), N.concat(u, w)),
                        N.bool_op("or", near, far))]
        for t in (u, w, h):
            cs += WK._guards(t, (64, 128))
        cs.append(_coupling(N.bv_op("bvxor", mid, target), 52))
        uv, wv = WK._guarded(TC._R[6], (64, 128)), WK._guarded(TC._R[7], (64, 128))
        wrong = _WIDE_WRONG                               # about 64 of the 512 bits
        a = (uv << 256 | wv) ^ wrong
        tv = (uv & ((1 << 128) - 1)) << 128 | wv >> 128
        return cs, {"a_hi": a >> 384, "a_mid": _all_wrong(a >> 128 & M256, tv, 52),
                    "a_lo": a & ((1 << 128) - 1), "u": uv, "w": wv,
                    "h": WK._guarded(TC._R[10], (64, 128))}
    if name == "odd":
        p, q, s = N.bv_var("p", 100), N.bv_var("q", 13), N.bv_var("s", 143)
        x, y, z = N.bv_var("x", 256), N.bv_var("y", 256), N.bv_var("z", 256)
        d, t = N.concat(p, q, s), N.bv_op("bvxor", x, y, z)
        cs = [N.eq(d, t), _coupling(N.bv_op("bvxor", d, t), 138)]
        for v in (x, y, z):
            cs += WK._guards(v, (64, 128))
        xv, yv, zv = (WK._guarded(r, (64, 128)) for r in (_R[0], _R[1], _R[3]))
        tv = xv ^ yv ^ zv
        dv = _all_wrong(tv ^ _R[2], tv, 138)              # about 128 bits away
        return cs, {"p": dv >> 156, "q": dv >> 143 & 0x1FFF, "s": dv & ((1 << 143) - 1),
                    "x": xv, "y": yv, "z": zv}
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
    """The case's aim table (the leaf order of a case is the same on both
    register layouts)."""
    A = RP.aim_table(trees(name), program(name))
    for a in (A.entries, A.pieces):
        a.setflags(write=False)
    return A


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
def reference(name, walkers=1, lanes=LANES, max_rounds=None, sync_every=8, aimed=True, seed=SEED):
    """walk_ref with the tree scoring through the oracle from the case's
    start; ``aimed``: with the case's aim table, else with plain moves."""
    prog = program(name)
    T = trees(name)
    res = RP.walk_ref(values_fn(name), default_leafgen(prog), consts_of(prog), starts(name, walkers),
                      T.roots, seed, lanes, MAX_ROUNDS[name] if max_rounds is None else max_rounds,
                      sync_every, score=RP.tree_scoring(T), aims=aims(name) if aimed else None)
    for a in (res.leaves, res.nfail, res.cost, res.trace):
        a.setflags(write=False)
    return res


def generator_hits(name, n):
    """Satisfying candidates among the default generator's first n."""
    cs = case(name)[0]
    prog = compile_constraints(cs, _built(name)[2], nreg=16)
    bits = evalref.run_gen(evalref.serialize(cs, prog), prog, SEED, 0, 0, n, per_root=True)
    return int(bits.all(axis=1).sum())

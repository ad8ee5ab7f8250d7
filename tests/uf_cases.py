"""Test infrastructure of the walk with aims for UF outputs
(tests/test_walk_uf.py, tests/test_gpu_walk_uf.py): the
crafted cases, their eval-form programs with root mask, atom mask, residual
probes and the arguments' chunks, their tables, the oracle's values as the
``values_fn`` of ``walk_ref``, and the reference runs, computed once per (case,
walkers, lanes, rounds, sync, table, seed).

Every case is in eval form with the default generator and carries the guards
of tests/walk_cases.py; the side that must move is one table entry of an
uninterpreted function f, and which entry is decided by the key leaves of the
walker's base.  Each start is ``target xor random``.
  hash    bvult(K, h) and bvule(h, t + 3), h = f(w) with its halves exchanged
          (two slot pieces; the pool's K + 1 is then no value of the entry
          that makes a model): w = concat(x, y), a 512-bit key of two chunks,
          t = p xor q with p, q and h guarded (the pool's 0 - 1 is all ones); K is a numeral with its 100 top
          bits set, and two more roots pin those bits of p to ones and of q
          to zeros, so a generated candidate has h below K, and t above it
          once the aims of §3.12 have set them.  The start has p and q
          right and h = (t + 1) xor random, below K.  No key leaf equals w at
          the start: the slot resolves to ``else``.  Of the orders' sides the
          UF side is the only one that resolves (K is a numeral, t + 3 a
          sum).  Entries: p and q (XOR, leaf pieces), h HIGH_STRICT (root 0),
          h LOW (root 1)
  shadow  f(a) = p xor q and f(b) = r xor s, all of a, b, p, q, r, s, f(a) and f(b) guarded
          (p = q = a and the pool's 0 would else do).
          The start's key leaves make entries 0 and 1 both equal a, so first
          match means entry 0; b hits nothing and reads ``else``.  Two XOR
          entries, whose run-time destinations differ: v0 and else
  rekey   `shadow` with the root c = d, from another start: entry 0's key is
          one bit away from a, so f(a) reads ``else`` as f(b) does; ``else``
          equals r xor s, so the aimed move on it fixes one root and breaks
          the other, while the plain move that makes the key equal a (a copy)
          lets f(a) read v0, which is closer to p xor q.  Round 0 has no aim
          and its best lane copies d to c (one root fewer); the re-keying
          copy is adopted in round 1, after the first resolution.  From then
          on the slot of f(a) must name v0: with the destinations of round 0
          the walk would write ``else`` for ever
  ckey    f(7) = p xor q and f(a) = r xor s, compiled with constant keys: f(7)
          is statically the leaf of the constant key's value (an XOR entry
          with a leaf piece), and f(a)'s slot has a CONST candidate that the
          start's a does not match

Chosen max_rounds and what was observed (one walker, 4096 lanes, seed SEED;
tests/test_walk_uf.py asserts (a) no model among the generator's lanes x
max_rounds candidates, (b) walk_ref with the table of §3.13 is still failing
after max_rounds, (c) with the tables of §3.14 it reaches nfail == 0 within
half of max_rounds):
  hash    max_rounds %d: the first round with nfail == 0 is round %d
  shadow  max_rounds %d: round %d
  rekey   max_rounds %d: round %d
  ckey    max_rounds %d: round %d
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
NAMES = ("hash", "shadow", "rekey", "ckey")
MAX_ROUNDS = {"hash": 16, "shadow": 32, "rekey": 32, "ckey": 32}
FIRST_ZERO = {"hash": 1, "shadow": 2, "rekey": 2, "ckey": 2}    # observed (see above)
__doc__ = __doc__ % tuple(v for n in NAMES for v in (MAX_ROUNDS[n], FIRST_ZERO[n]))

_rng = np.random.default_rng(0x7566)
_R = [int.from_bytes(_rng.bytes(32), "little") for _ in range(16)]
M256 = (1 << 256) - 1
AT = (64, 128)
KEY_BIT = 32


def _f(arg):
    return N.apply_uf("f", arg.width, 256, arg)


def _swap(v):
    """The 256-bit term v with its halves exchanged."""
    return N.concat(N.extract(127, 0, v), N.extract(255, 128, v))


def _case(name):
    """(constraints, start {leaf name: value}); a leaf the start does not
    name starts at the value of ``"*"``."""
    var = lambda s, w=256: N.bv_var(s, w)
    if name == "hash":
        x, y, p, q = var("x"), var("y"), var("p"), var("q")
        ones = (1 << 100) - 1
        K = ones << 156 | _R[0] >> 120
        fw, t = _swap(_f(N.concat(x, y))), N.bv_op("bvxor", p, q)
        cs = [N.bv_cmp("bvult", N.bv_num(K, 256), fw),
              N.bv_cmp("bvule", fw, N.bv_op("bvadd", t, N.bv_num(3, 256))),
              N.eq(N.extract(255, 156, p), N.bv_num(ones, 100)),
              N.eq(N.extract(255, 156, q), N.bv_num(0, 100))]
        for v in (p, q, fw):
            cs += WK._guards(v, AT)
        low = (1 << 156) - 1
        pv = ones << 156 | WK._guarded(_R[2], AT) & low
        qv = (WK._guarded(_R[1], AT) ^ (0x1111 << 64 | 0x1111 << 128)) & low
        tv = pv ^ qv
        sw = (tv + 1) ^ _R[3]                                        # target xor random
        ev = (sw << 128 | sw >> 128) & M256
        assert K < tv and sw < K
        start = {"x": _R[4], "y": _R[5], "p": pv, "q": qv, "f#else#0": ev, "*": _R[6]}
        return cs, start
    if name in ("shadow", "rekey"):
        a, b = var("a"), var("b")
        p, q, r, s = (var(c) for c in "pqrs")
        cs = [N.eq(_f(a), N.bv_op("bvxor", p, q)), N.eq(_f(b), N.bv_op("bvxor", r, s))]
        for v in (a, b, p, q, r, s, _f(a), _f(b)):
            cs += WK._guards(v, AT)
        if name == "rekey":
            c, d = var("c"), var("d")
            cs += [N.eq(c, d)] + WK._guards(c, AT)
        av, bv, pv, rv = (WK._guarded(_R[i], AT) for i in range(4))
        qv = WK._guarded(_R[4], AT) ^ (0x1111 << 64 | 0x1111 << 128)     # p xor q: windows 0x1111
        sv = WK._guarded(_R[5], AT) ^ (0x2222 << 64 | 0x2222 << 128)
        start = {"a": av, "b": bv, "p": pv, "q": qv, "r": rv, "s": sv, "*": _R[9]}
        if name == "shadow":
            start.update({"f#k0#0": av, "f#k1#0": av, "f#v0#0": WK._guarded(pv ^ qv ^ _R[6] >> 56, AT),
                          "f#v1#0": _R[7], "f#else#0": WK._guarded(rv ^ sv ^ _R[8] >> 56, AT)})
        else:
            # v0 is some 80 bits from p xor q, else (= r xor s) about 128
            start.update({"f#k0#0": av ^ (1 << KEY_BIT), "f#k1#0": _R[7],
                          "f#v0#0": WK._guarded(pv ^ qv ^ _R[6] >> 96, AT),
                          "f#v1#0": _R[10], "f#else#0": rv ^ sv,
                          "c": WK._guarded(_R[11], AT), "d": WK._guarded(_R[12], AT)})
        return cs, start
    if name == "ckey":
        a = var("a")
        p, q, r, s = (var(c) for c in "pqrs")
        cs = [N.eq(_f(N.bv_num(7, 256)), N.bv_op("bvxor", p, q)),
              N.eq(_f(a), N.bv_op("bvxor", r, s))]
        for v in (a, p, q, r, s, _f(N.bv_num(7, 256)), _f(a)):
            cs += WK._guards(v, AT)
        av, pv, rv = (WK._guarded(_R[i], AT) for i in (10, 11, 12))
        qv = WK._guarded(_R[13], AT) ^ (0x1111 << 64 | 0x1111 << 128)
        sv = WK._guarded(_R[14], AT) ^ (0x2222 << 64 | 0x2222 << 128)
        start = {"a": av, "p": pv, "q": qv, "r": rv, "s": sv, "f#c0#0": WK._guarded(pv ^ qv ^ _R[6] >> 56, AT),
                 "f#else#0": WK._guarded(rv ^ sv ^ _R[8] >> 56, AT), "*": _R[9]}
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
        apps, uprobes = RP.uf_probes(trees)
    for a in (trees.roots, trees.atoms, trees.code):
        a.setflags(write=False)
    return cs, start, mask, amask, trees, tuple(apps), tuple(uprobes)


def case(name):
    """(constraints, start assignment {leaf name: value})."""
    return _built(name)[:2]


def trees(name):
    return _built(name)[4]


def apps(name):
    return _built(name)[5]


@functools.lru_cache(maxsize=None)
def program(name, nreg=16):
    """The case's eval-form program: root mask, atom mask, the trees'
    residuals, the arguments' chunks (`ckey`: with constant keys)."""
    cs, _, mask, amask, T, _, up = _built(name)
    return compile_constraints(cs, mask + amask + list(T.probes) + list(up), nreg=nreg,
                               const_keys=name == "ckey")


@functools.lru_cache(maxsize=None)
def tables(name):
    """(Bounds, Ufs) of §3.14, built outside the scope the nodes were built in."""
    B, U = RP.uf_table(case(name)[0], trees(name), program(name), apps(name))
    for a in (B.entries, B.pieces, B.fixed, U.slots, U.funcs, U.cands, U.ukeys):
        a.setflags(write=False)
    return B, U


@functools.lru_cache(maxsize=None)
def bounds(name):
    """The case's table of §3.13: no application resolves."""
    return RP.bound_table(case(name)[0], trees(name), program(name))


def n_before(name):
    """The probes in front of the U rows."""
    _, _, mask, amask, T, _, _ = _built(name)
    return len(mask) + len(amask) + len(T.probes)


def view(name, nreg=16):
    """What the walk loads: the program with its U rows (``repair.uf_view``)."""
    U = tables(name)[1]
    return RP.uf_view(program(name, nreg), n_before(name) + U.n_arg_rows, U.keep)


def leaf_rows(prog, values):
    out = np.zeros((len(prog.leaves), 8), dtype=np.uint32)
    for i, leaf in enumerate(prog.leaves):
        v = values.get(leaf.name if leaf.kind != "var" else leaf.source, values["*"])
        out[i] = np.frombuffer((v & ((1 << leaf.width) - 1)).to_bytes(32, "little"), dtype="<u4")
    return out


def start_rows(name):
    return leaf_rows(program(name), case(name)[1])


def starts(name, walkers):
    """(walkers, n_leaves, 8): the case's start for every walker."""
    return np.repeat(start_rows(name)[None], walkers, axis=0)


consts_of = WK.consts_of


@functools.lru_cache(maxsize=None)
def _serialized(name):
    cs, _, _, _, T, _, up = _built(name)
    return evalref.serialize(cs, program(name), list(T.atom_nodes) + list(T.probes) + list(up))


def values_fn(name, urows=True):
    """SoA leaves (n_leaves, 8, n) -> (root verdicts (n, n_roots) bool, atom
    verdicts (n, n_atoms) bool, residual values (n_resid, 8, n) u32, U rows
    (n_urows, 8, n) u32: the arguments' chunks; eval form has no key row),
    from the oracle alone.  ``urows`` False: the first three."""
    S, prog = _serialized(name), program(name)
    cs, _, _, _, T, _, up = _built(name)
    nodes = list(cs) + list(T.atom_nodes) + list(T.probes) + list(up)
    records = [S.node_index[n.id] for n in nodes]
    n_c, n_a, n_r = len(cs), len(T.atom_nodes), len(T.probes)

    def fn(soa):
        _, vals = evalref.run_nodes_soa(S, prog, np.ascontiguousarray(soa), records=records,
                                        chunk=256)
        bits = (vals[:, :n_c, 0] & np.uint64(1)).astype(bool)
        abits = (vals[:, n_c:n_c + n_a, 0] & np.uint64(1)).astype(bool)
        out = (bits, abits, TC._rows(vals[:, n_c + n_a:n_c + n_a + n_r]))
        return out + (TC._rows(vals[:, n_c + n_a + n_r:]),) if urows else out
    return fn


@functools.lru_cache(maxsize=None)
def reference(name, walkers=1, lanes=LANES, max_rounds=None, sync_every=8, uf=True, seed=SEED):
    """walk_ref with the tree scoring through the oracle from the case's
    start; ``uf``: with the case's tables of §3.14, else with the table of
    §3.13."""
    prog = program(name)
    T = trees(name)
    if uf:
        B, U = tables(name)
        kw = dict(bounds=B, ufs=U)
    else:
        kw = dict(bounds=bounds(name))
    res = RP.walk_ref(values_fn(name, uf), default_leafgen(prog), consts_of(prog),
                      starts(name, walkers), T.roots, seed, lanes,
                      MAX_ROUNDS[name] if max_rounds is None else max_rounds, sync_every,
                      score=RP.tree_scoring(T), **kw)
    for a in (res.leaves, res.nfail, res.cost, res.trace):
        a.setflags(write=False)
    return res


def generator_hits(name, n):
    """Satisfying candidates among the default generator's first n."""
    cs = case(name)[0]
    prog = compile_constraints(cs, _built(name)[2], nreg=16, const_keys=name == "ckey")
    bits = evalref.run_gen(evalref.serialize(cs, prog), prog, SEED, 0, 0, n, per_root=True)
    return int(bits.all(axis=1).sum())

"""Test infrastructure of the scored walk (tests/test_walk.py,
tests/test_gpu_walk.py): the crafted cases — constraints, a
start, lanes and a round budget — their eval-form programs with mask and
residual probes, the oracle's verdict bits and residual values as the
``values_fn`` of ``walk_ref``, and the reference runs, computed once per
(case, walkers, lanes, rounds, sync).

Every case is in eval form with the default generator and carries the guards
of tests/repair_cases.py (two 16-bit windows of a leaf, neither 0 nor 0xFFFF:
every boundary and pool value of the generator has one window all zeros or
all ones).  Each is one constraint short of a model but many moves away:
  hamming    x ^ y == z over three 256-bit leaves, no constant on either
             side, guards on x, y and z (so neither the generator's zeros nor
             a copy plus a pool value make a model); the start is random,
             about half of the 256 bits away
  magnitude  lo < y - x and y - x < hi over two 64-bit leaves, hi - lo = 4,
             guards on x; the start has y - x = 2^40 + 1
  mixed      257 roots, two mask probes: 250 one-bit equalities on a 256-bit
             x and not (z == 0) (the `wide` shape of tests/repair_cases.py;
             a one-bit equality's distance is identically 1, so residuals()
             makes those roots FLAT), u ^ v == w over three 64-bit leaves,
             none of them 0, and the window of `magnitude` on q - p; the
             start has six bits of x wrong, z = 0, u, v, w random and q - p =
             2^40 + 1

Chosen max_rounds and what was observed (one walker, 4096 lanes, seed SEED;
tests/test_walk.py asserts (a) no model among the generator's lanes x
max_rounds candidates, (b) repair_ref still fails after max_rounds, (c)
walk_ref reaches nfail == 0 within half of max_rounds):
  hamming    max_rounds %d: walk_ref's first round with nfail == 0 is round %d
  magnitude  max_rounds %d: round %d
  mixed      max_rounds %d: round %d
"""

import functools

import numpy as np

from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import default_leafgen
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N
from oracle import evalref

SEED = 0x77616C6B
LANES = 4096
NAMES = ("hamming", "magnitude", "mixed")
MAX_ROUNDS = {"hamming": 96, "magnitude": 16, "mixed": 64}
FIRST_ZERO = {"hamming": 41, "magnitude": 2, "mixed": 20}     # observed (see above)
__doc__ = __doc__ % tuple(v for n in NAMES for v in (MAX_ROUNDS[n], FIRST_ZERO[n]))

_rng = np.random.default_rng(0x77616C6B)
_R = [int.from_bytes(_rng.bytes(32), "little") for _ in range(8)]
_WIDE_BITS = int.from_bytes(_rng.bytes(32), "little")
LO, HI = 1000, 1004
M64 = (1 << 64) - 1


def _eqc(a, v):
    return N.eq(a, N.bv_num(v, a.width))


def _guards(x, at):
    """Neither window of x (16 bits from each of ``at``) is 0 or 0xFFFF."""
    return [N.bool_op("not", _eqc(N.extract(lo + 15, lo, x), v)) for lo in at
            for v in (0, 0xFFFF)]


def _guarded(v, at):
    """v with the windows set to values the guards admit."""
    for lo, k in zip(at, (0x1234, 0x4321)):
        v = v & ~(0xFFFF << lo) | (k << lo)
    return v


def _window(p, q):
    d = N.bv_op("bvsub", q, p)
    return [N.bv_cmp("bvult", N.bv_num(LO, 64), d), N.bv_cmp("bvult", d, N.bv_num(HI, 64))]


def _case(name):
    if name == "hamming":
        x, y, z = (N.bv_var(s, 256) for s in "xyz")
        cs = [N.eq(N.bv_op("bvxor", x, y), z)]
        for v in (x, y, z):
            cs += _guards(v, (64, 128))
        return cs, {s: _guarded(r, (64, 128)) for s, r in zip("xyz", _R)}
    if name == "magnitude":
        x, y = N.bv_var("x", 64), N.bv_var("y", 64)
        cs = _window(x, y) + _guards(x, (16, 40))
        xv = _guarded(_R[3] & M64, (16, 40))
        return cs, {"x": xv, "y": (xv + (1 << 40) + 1) & M64}
    if name == "mixed":
        x, z = N.bv_var("x", 256), N.bv_var("z", 8)
        u, v, w = (N.bv_var(s, 64) for s in "uvw")
        p, q = N.bv_var("p", 64), N.bv_var("q", 64)
        cs = [_eqc(N.extract(i, i, x), (_WIDE_BITS >> i) & 1) for i in range(250)]
        cs.append(N.bool_op("not", _eqc(z, 0)))
        cs.append(N.eq(N.bv_op("bvxor", u, v), w))
        cs += [N.bool_op("not", _eqc(t, 0)) for t in (u, v, w)]
        cs += _window(p, q)
        assert len(cs) == 257
        wrong = sum(1 << i for i in (0, 31, 32, 100, 200, 249))
        pv = _R[7] & M64
        return cs, {"x": _WIDE_BITS ^ wrong, "z": 0, "u": _R[4] & M64, "v": _R[5] & M64,
                    "w": _R[6] & M64, "p": pv, "q": (pv + (1 << 40) + 1) & M64}
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _built(name):
    """The case's nodes, built in one order inside a scope of their own: a
    program's schedule follows the order of the node ids, and `mixed` fills
    the compiler's spill budget on the 11-slot layout (its 257 mask bits are
    live at once), so what a process built before must not reorder them."""
    with N.fresh_scope():
        cs, start = _case(name)
        probes, table = RP.residuals(cs)
        mask = CS.mask_probes(cs)
    table.setflags(write=False)
    return cs, start, mask, tuple(probes), table


def case(name):
    """(constraints, start assignment {symbol: value})."""
    return _built(name)[:2]


def scoring(name, flat=False):
    """(residual probe nodes, table) of the case; ``flat``: no residuals,
    every root FLAT (the count alone)."""
    cs, _, _, probes, table = _built(name)
    return ((), RP.flat_table(len(cs))) if flat else (probes, table)


@functools.lru_cache(maxsize=None)
def program(name, nreg=16, flat=False):
    """The case's eval-form program: mask probes, then residual probes."""
    cs, _, mask, _, _ = _built(name)
    return compile_constraints(cs, mask + list(scoring(name, flat)[0]), nreg=nreg)


def leaf_rows(prog, values):
    out = np.zeros((len(prog.leaves), 8), dtype=np.uint32)
    for i, leaf in enumerate(prog.leaves):
        v = values[leaf.source] & ((1 << leaf.width) - 1)
        out[i] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    return out


def start_rows(name):
    return leaf_rows(program(name), case(name)[1])


def starts(name, walkers):
    """(walkers, n_leaves, 8): the case's start for every walker."""
    return np.repeat(start_rows(name)[None], walkers, axis=0)


def consts_of(prog):
    return np.ascontiguousarray(prog.consts, dtype=np.uint32).reshape(-1, 8)


@functools.lru_cache(maxsize=None)
def _serialized(name, flat=False):
    cs, _ = case(name)
    return evalref.serialize(cs, program(name, 16, flat), scoring(name, flat)[0])


def values_fn(name, flat=False):
    """SoA leaves (n_leaves, 8, n) -> ((n, n_roots) bool verdicts, (n_resid, 8,
    n) u32 residual values), from the oracle alone: one pass over the DAG, the
    values of the root records and of the residual records kept."""
    S, prog = _serialized(name, flat), program(name, 16, flat)
    cs, _ = case(name)
    resid = scoring(name, flat)[0]
    records = [S.node_index[c.id] for c in cs] + [S.node_index[r.id] for r in resid]

    def fn(soa):
        soa = np.ascontiguousarray(soa)
        _, vals = evalref.run_nodes_soa(S, prog, soa, records=records, chunk=256)
        bits = (vals[:, :len(cs), 0] & np.uint64(1)).astype(bool)
        r64 = np.ascontiguousarray(vals[:, len(cs):, :4]).view("<u4")          # (n, n_resid, 8)
        return bits, np.ascontiguousarray(r64.transpose(1, 2, 0))
    return fn


def bits_fn(name):
    fn = values_fn(name, True)
    return lambda soa: fn(soa)[0]


@functools.lru_cache(maxsize=None)
def reference(name, walkers=1, lanes=LANES, max_rounds=None, sync_every=8, flat=False):
    """walk_ref through the oracle from the case's start."""
    prog = program(name, 16, flat)
    res = RP.walk_ref(values_fn(name, flat), default_leafgen(prog), consts_of(prog),
                      starts(name, walkers), scoring(name, flat)[1], SEED, lanes,
                      MAX_ROUNDS[name] if max_rounds is None else max_rounds, sync_every)
    for a in (res.leaves, res.nfail, res.cost, res.trace):
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def count_reference(name):
    """repair_ref (the count alone) from the same start, same budget."""
    prog = program(name, 16, True)
    return RP.repair_ref(bits_fn(name), default_leafgen(prog), consts_of(prog), start_rows(name),
                         SEED, LANES, MAX_ROUNDS[name], 8)


def generator_hits(name, n):
    """Satisfying candidates among the default generator's first n."""
    bits = evalref.run_gen(_serialized(name, True), program(name, 16, True), SEED, 0, 0, n,
                           per_root=True)
    return int(bits.all(axis=1).sum())

"""Test infrastructure of the local search (tests/test_repair.py,
tests/test_gpu_repair.py): the crafted cases — constraints, a nearly
satisfying start, lanes and round budget — their eval-form masked programs,
the oracle's per-constraint bits as the ``bits_fn`` of ``repair_ref``, and the
reference runs, computed once per (case, lanes, rounds, sync).

Every case is in eval form with the default generator, and chosen so that
  - ``repair_ref`` reaches nfail == 0 within half of the case's max_rounds, and
  - the default generator finds no satisfying candidate among lanes x
    max_rounds candidates
(tests/test_repair.py checks both).  What was chosen where the issue left
room:
  bytes   one 256-bit x, 8 one-byte fields (bytes 0, 4, .., 28) instead of 32:
          a byte move hits one given byte with one given value once in
          6 * 32 * 256 draws, so 32 fields need more than the 32 rounds half
          of the budget allows; the start has four of the eight right
  twins   x == y and not (x == 0) as given, plus four guards on two 16-bit
          windows of x (neither 0 nor 0xFFFF): every boundary and pool value
          of the generator has one window all zeros or all ones, so the
          generator's equal pairs are no models, and not the census's best
          candidate either
  step    as given, plus the same four guards: without them the generator's
          pair x = 2^255 - 1, y = 2^255 is a model (one hit in 2^18
          candidates), and its small consecutive pairs (0, 1), (1, 2) fail
          the byte alone, a best candidate no single walker leaves; the
          start is y = x + 1 + 2^40 with the byte set
  wide    256 one-bit roots on a 256-bit x and not (z == 0) on an 8-bit z:
          257 roots, two mask probes; the start has six bits wrong and z = 0
  narrow  33 leaves of width 1..33, each equal to a constant; the start has
          five leaves off by one bit
"""

import functools

import numpy as np

from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import default_leafgen
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N
from oracle import evalref

SEED = 0x7265
LANES = 4096
MAX_ROUNDS = 64
NAMES = ("bytes", "twins", "step", "wide", "narrow")

_rng = np.random.default_rng(0x6D67)
_BYTES_K = [int(v) for v in _rng.permutation(np.arange(2, 250))[:8]]
_WIDE_BITS = int.from_bytes(_rng.bytes(32), "little")
_NARROW_C = [int.from_bytes(_rng.bytes(8), "little") & ((1 << w) - 1) | (1 << (w - 1))
             for w in range(1, 34)]
_X0 = int.from_bytes(_rng.bytes(32), "little")
_Y0 = int.from_bytes(_rng.bytes(32), "little")


def _eqc(a, v):
    return N.eq(a, N.bv_num(v, a.width))


@functools.lru_cache(maxsize=None)
def case(name):
    """(constraints, start assignment {symbol: value})."""
    if name == "bytes":
        x = N.bv_var("x", 256)
        at = [32 * i for i in range(8)]
        cs = [_eqc(N.extract(lo + 7, lo, x), k) for lo, k in zip(at, _BYTES_K)]
        v = _X0
        for lo, k in list(zip(at, _BYTES_K))[:4]:
            v = v & ~(0xFF << lo) | (k << lo)
        for lo, k in list(zip(at, _BYTES_K))[4:]:
            v = v & ~(0xFF << lo) | ((k ^ 0x55) << lo)
        return cs, {"x": v}
    if name == "twins":
        x, y = N.bv_var("x", 256), N.bv_var("y", 256)
        a, b = N.extract(79, 64, x), N.extract(143, 128, x)
        cs = [N.eq(x, y), N.bool_op("not", _eqc(x, 0))]
        cs += [N.bool_op("not", _eqc(w, v)) for w in (a, b) for v in (0, 0xFFFF)]
        return cs, {"x": _X0 | (0x1234 << 64) | (0x4321 << 128), "y": _Y0}
    if name == "step":
        x, y = N.bv_var("x", 256), N.bv_var("y", 256)
        a, b = N.extract(79, 64, x), N.extract(143, 128, x)
        cs = [_eqc(N.bv_op("bvsub", y, x), 1), N.bv_cmp("bvult", x, y),
              _eqc(N.extract(255, 248, x), 0x7F)]
        cs += [N.bool_op("not", _eqc(w, v)) for w in (a, b) for v in (0, 0xFFFF)]
        xv = (_X0 & ((1 << 248) - 1) | (0x7F << 248)) | (0x1234 << 64) | (0x4321 << 128)
        return cs, {"x": xv, "y": xv + 1 + (1 << 40)}
    if name == "wide":
        x, z = N.bv_var("x", 256), N.bv_var("z", 8)
        cs = [_eqc(N.extract(i, i, x), (_WIDE_BITS >> i) & 1) for i in range(256)]
        cs.append(N.bool_op("not", _eqc(z, 0)))
        wrong = sum(1 << i for i in (0, 31, 32, 100, 200, 255))
        return cs, {"x": _WIDE_BITS ^ wrong, "z": 0}
    if name == "narrow":
        vs = [N.bv_var("v%02d" % w, w) for w in range(1, 34)]
        cs = [_eqc(v, c) for v, c in zip(vs, _NARROW_C)]
        start = {"v%02d" % w: c for w, c in zip(range(1, 34), _NARROW_C)}
        for w in (1, 8, 17, 32, 33):
            start["v%02d" % w] ^= 1 << (w // 2)
        return cs, start
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def masked_program(name, nreg=16):
    cs, _ = case(name)
    return compile_constraints(cs, CS.mask_probes(cs), nreg=nreg)


def leaf_rows(prog, values):
    """(n_leaves, 8) u32 of an assignment {symbol: value} (one leaf per
    symbol: no case has a symbol above 256 bits)."""
    out = np.zeros((len(prog.leaves), 8), dtype=np.uint32)
    for i, leaf in enumerate(prog.leaves):
        v = values[leaf.source] & ((1 << leaf.width) - 1)
        out[i] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    return out


def leaf_values(prog, rows):
    return {leaf.source: int.from_bytes(np.ascontiguousarray(rows[i], dtype="<u4").tobytes(),
                                        "little") for i, leaf in enumerate(prog.leaves)}


def start_rows(name):
    return leaf_rows(masked_program(name), case(name)[1])


def consts_of(prog):
    return np.ascontiguousarray(prog.consts, dtype=np.uint32).reshape(-1, 8)


@functools.lru_cache(maxsize=None)
def _serialized(name):
    return evalref.serialize(case(name)[0], masked_program(name))


def bits_fn(name):
    """SoA leaves (n_leaves, 8, n) -> (n, n_constraints) bool, from the
    oracle alone."""
    S, prog = _serialized(name), masked_program(name)
    return lambda soa: evalref.run_leaves_soa(S, prog, np.ascontiguousarray(soa), per_root=True)


@functools.lru_cache(maxsize=None)
def reference(name, lanes=LANES, max_rounds=MAX_ROUNDS, sync_every=8):
    """repair_ref through the oracle from the case's start."""
    prog = masked_program(name)
    res = RP.repair_ref(bits_fn(name), default_leafgen(prog), consts_of(prog), start_rows(name),
                        SEED, lanes, max_rounds, sync_every)
    res.leaves.setflags(write=False)
    res.trace.setflags(write=False)
    return res


def generator_hits(name, n):
    """Satisfying candidates among the default generator's first n."""
    bits = evalref.run_gen(_serialized(name), masked_program(name), SEED, 0, 0, n, per_root=True)
    return int(bits.all(axis=1).sum())

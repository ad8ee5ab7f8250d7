"""Operands of the full-width-divisor division tests (tests/test_div_fullwidth.py
on the assembly simulator, tests/test_gpu_div_fullwidth.py on the GPU): one
division per program, 256 lanes = four waves of 64.

* wave (a): every divisor magnitude keeps a nonzero top limb (bits 224..255),
  so the wave takes asmgen._udivrem_full: top limbs 1, 0x7fffffff, 0x80000000
  and 0xffffffff (a normalising shift of 31, 1, 0, 0 bits), dividends below,
  equal to and above the divisor, dag_cases.hard_division_pair pairs with a
  full-width divisor, and pairs of that shape with the top limb 1, whose
  quotient estimate is often two too big (``_hard_pairs`` says why both);
* wave (b): the same with one lane's divisor narrowed to 224 bits (the wave
  takes the general path);
* wave (c): the same with one zero divisor;
* wave (d): signed operands of all four sign combinations, INT_MIN / -1 and
  its neighbours.

The signed operators see magnitudes, so their waves (a)-(c) are built from
magnitudes below 2^255 (the hard pairs halved; INT_MIN alone has the top limb
0x80000000) under all four sign combinations.
"""

import random

import dag_cases
from mythril_amd.smt import node as N
from oracle import smtlib_ref as R

OPS = ("bvudiv", "bvurem", "bvsdiv", "bvsrem", "bvsmod")
SIGNED = ("bvsdiv", "bvsrem", "bvsmod")
M256 = (1 << 256) - 1
INT_MIN = 1 << 255
NARROW_LANE, ZERO_LANE = 30, 9          # a hard pair's divisor; (y + 1) / y
N_HARD = 36


def magnitude(v: int, signed: bool) -> int:
    return (1 << 256) - v if signed and v >> 255 else v


def _hard_pairs(rng, signed):
    """dag_cases.hard_division_pair pairs with a full-width divisor (halved
    for the signed operators), then pairs of the same shape one bit above
    224: a full-width divisor leaves a quotient below 2^32 / (top limb), and
    an estimate two too big needs a quotient digit of about 2^31 or more, so
    it needs the top limb 1 (hard_division_pair's own full-width divisors
    have the top bit set: quotient 0 or 1, estimate exact or one too big).
    A signed dividend's magnitude stays below 2^255, its quotient below
    2^31: those lanes reach one add-back, never two."""
    out = []
    while len(out) < N_HARD // 3:
        x, y = dag_cases.hard_division_pair(rng)
        if signed:
            x, y = x >> 1, y >> 1
        if y >> 224:
            out.append((x, y))
    cap = INT_MIN - 1 if signed else M256
    while len(out) < N_HARD:
        y = 1 << 224 | (rng.getrandbits(31) << 193 if rng.random() < 0.5 else 0) | ((1 << 193) - 1)
        m = min(rng.getrandbits(32) | 1 << 31, cap // y)
        out.append((y * m - rng.getrandbits(40), y))
    return out


def magnitude_pairs(signed: bool):
    """64 (dividend, divisor) magnitude pairs of wave (a)."""
    rng = random.Random(21 + signed)
    tops = (1, 0x7FFFFFFF, 0x40000000, 0x7FFFFFFE) if signed else (1, 0x7FFFFFFF, 0x80000000,
                                                                   0xFFFFFFFF)
    cap = INT_MIN - 1 if signed else M256
    out = []
    for top in tops:
        y = top << 224 | rng.getrandbits(224)
        out += [(y - 1, y), (y, y), (min(y + 1, cap), y), (cap, y), (rng.getrandbits(100), y),
                (cap, top << 224), (min(2 * y + 1, cap), y)]
    out += _hard_pairs(rng, signed)
    assert len(out) == 64
    return out


def wave_a(op: str):
    """64 (x, y) operand values of wave (a) for ``op``."""
    signed = op in SIGNED
    pairs = magnitude_pairs(signed)
    if not signed:
        return pairs
    out = []
    for lane, (x, y) in enumerate(pairs):
        out.append(((-x if lane & 1 else x) & M256, (-y if lane & 2 else y) & M256))
    # INT_MIN: the one magnitude with the top limb 0x80000000 (no bit shift)
    out[3] = (out[3][0], INT_MIN)
    out[10] = (INT_MIN, INT_MIN)
    out[17] = (INT_MIN, out[17][1])
    return out


def waves(op: str):
    """The four waves of ``op``: {name: 64 (x, y)}."""
    signed = op in SIGNED
    a = wave_a(op)
    b = list(a)
    x, y = b[NARROW_LANE]
    m = magnitude(y, signed) & ((1 << 224) - 1) or 1
    b[NARROW_LANE] = (x, (-m if signed and y >> 255 else m) & M256)
    c = list(a)
    c[ZERO_LANE] = (c[ZERO_LANE][0], 0)
    rng = random.Random(77)
    d = []
    for lane in range(64):
        x, y = rng.getrandbits(255), rng.getrandbits(rng.choice((255, 250, 225, 224, 130, 20)))
        d.append(((-x if lane & 1 else x) & M256, (-y if lane & 2 else y) & M256))
    d[0] = (INT_MIN, M256)                       # INT_MIN / -1
    d[1] = (INT_MIN, 1)
    d[2] = (M256, INT_MIN)
    d[3] = (INT_MIN, INT_MIN)
    d[4] = (INT_MIN - 1, INT_MIN)
    d[6] = (INT_MIN + 1, M256)
    return {"a": a, "b": b, "c": c, "d": d}


def program_nodes(op: str):
    """(x, y, probe) of the one-division program of ``op``."""
    x, y = N.bv_var("x", 256), N.bv_var("y", 256)
    return x, y, N.bv_op(op, x, y)


_WANT = {}


def expected(op: str, name: str):
    """oracle/smtlib_ref.py values of wave ``name`` of ``op`` (computed once)."""
    if (op, name) not in _WANT:
        _, _, probe = program_nodes(op)
        _WANT[op, name] = [R.evaluate([probe], R.Assignment({"x": x, "y": y}))[0]
                           for x, y in waves(op)[name]]
    return _WANT[op, name]

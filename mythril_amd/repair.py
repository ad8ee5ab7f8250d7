"""Greedy local search from a missed search's best candidate.

The witness search draws every candidate afresh, so it never looks at a
neighbour of a candidate that came close.  The census (``census.py``) names
that candidate; this module walks from it: per round, ``lanes`` neighbours of
the current base assignment — one or two leaves changed by a small move — are
evaluated, and the neighbour with the fewest failing constraints becomes the
next base if it fails strictly fewer than the base does.  The loop runs on
the device (``mg_repair``, ``csrc/mg_repair.hip``); :func:`mutate_ref` is the
specification of its move function (``csrc/mg_repair.h``) and
:func:`repair_ref` of the loop, bit for bit.

Soundness is the caller's as for any witness: :func:`repair_group` accepts an
assignment only after one fresh evaluation of the full masked program shows
the root and every mask bit set, and ``get_model`` still verifies it with z3.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np

M64 = (1 << 64) - 1
# the constants of csrc/mg_repair.h
CR, CJ, CD = 0xD6E8FEB86659FD93, 0xA0761D6478BD642F, 0xE7037ED1A0B428DB
GOLD, MIX = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9
KINDS = 6
FLIP, STEP, BYTE, LIMB, POOL, COPY = range(KINDS)
MAX_LANES, MAX_ROUNDS = 1 << 20, 1 << 16


def _hash(seed: int, r: int, j: np.ndarray, draw: int) -> np.ndarray:
    """The generator's v9 mix of (seed, r, j, draw): u64 per lane."""
    with np.errstate(over="ignore"):
        s = (np.uint64(seed & M64) ^ np.uint64((r * CR) & M64) ^ (j.astype(np.uint64) * np.uint64(CJ))
             ^ np.uint64(((draw + 1) * CD) & M64))
        s = s + np.uint64(GOLD)
        z = (s ^ (s >> np.uint64(32))) * np.uint64(MIX)
        return z ^ (z >> np.uint64(32))


def _mulhi(a: np.ndarray, n) -> np.ndarray:
    return ((a.astype(np.uint64) * np.asarray(n, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


def _ints(rows: np.ndarray) -> List[int]:
    b = np.ascontiguousarray(rows, dtype="<u4").tobytes()
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(rows))]


def _gen_fields(leafgen):
    return (np.array([g.width for g in leafgen], dtype=np.int64),
            np.array([g.pool_off for g in leafgen], dtype=np.int64),
            np.array([g.pool_n for g in leafgen], dtype=np.int64))


def moves_ref(leafgen, consts, base, seed: int, r: int, lanes: int):
    """Per lane of round ``r``, its moves as a list of (leaf, kind, value):
    leaf ``leaf`` takes ``value`` (a Python int, masked to the leaf's width),
    in order; the second move of a lane sees the result of the first.  Lane
    0 has none, lanes below ``lanes // 2`` one, the others two."""
    width, pool_off, pool_n = _gen_fields(leafgen)
    n_leaves = len(width)
    if n_leaves == 0 or not 1 <= lanes <= MAX_LANES or not 0 <= r < MAX_ROUNDS:
        raise ValueError("moves_ref: no leaves, lanes outside 1..2^20 or a round outside 0..2^16-1")
    cvals = _ints(np.asarray(consts, dtype=np.uint32).reshape(-1, 8))
    bvals = _ints(np.asarray(base, dtype=np.uint32).reshape(n_leaves, 8))
    j = np.arange(lanes, dtype=np.int64)
    n_moves = np.where(j == 0, 0, np.where(j < lanes // 2, 1, 2))
    draws = []
    for m in range(2):
        h0, h1 = _hash(seed, r, j, 2 * m), _hash(seed, r, j, 2 * m + 1)
        lo0, hi0 = h0 & np.uint64(0xFFFFFFFF), h0 >> np.uint64(32)
        a, c = h1 & np.uint64(0xFFFFFFFF), h1 >> np.uint64(32)
        leaf = _mulhi(lo0, n_leaves)
        w = width[leaf]
        draws.append((leaf.tolist(), _mulhi(hi0, KINDS).tolist(), a.tolist(), c.tolist(),
                      _mulhi(a, w).tolist(), _mulhi(a, (w + 7) // 8).tolist(),
                      _mulhi(a, (w + 31) // 32).tolist(), _mulhi(a, np.maximum(pool_n[leaf], 1)).tolist(),
                      _mulhi(c, 3).tolist(), _mulhi(a, n_leaves).tolist()))
    out = []
    for lane in range(lanes):
        cur = {}
        row = []
        for m in range(int(n_moves[lane])):
            leaf, kind, a, c, b, byte, limb, e, delta, other = (d[lane] for d in draws[m])
            w = int(width[leaf])
            v = cur.get(leaf, bvals[leaf])
            if kind == FLIP:
                v ^= 1 << b
            elif kind == STEP:
                v = v - (1 << b) if c & 1 else v + (1 << b)
            elif kind == BYTE:
                v = (v & ~(0xFF << (8 * byte))) | ((c & 0xFF) << (8 * byte))
            elif kind == LIMB:
                v = (v & ~(0xFFFFFFFF << (32 * limb))) | (c << (32 * limb))
            elif kind == POOL:
                if pool_n[leaf] > 0:
                    v = (cvals[int(pool_off[leaf]) + e] + delta - 1) % (1 << 256)
                else:
                    v = (0, 1, 1 << (w - 1), (1 << w) - 1)[c & 3]
            else:
                v = cur.get(other, bvals[other])
            v &= (1 << w) - 1
            cur[leaf] = v
            row.append((leaf, kind, v))
        out.append(row)
    return out


def mutate_ref(leafgen, consts, base, seed: int, r: int, lanes: int) -> np.ndarray:
    """``[n_leaves][8][lanes]`` u32: the neighbours of ``base``
    (``[n_leaves][8]`` u32) that round ``r`` evaluates — the specification of
    ``csrc/mg_repair.h``.  ``leafgen``: the program's leaf table (width,
    pool_off, pool_n), ``consts``: its constant table ``[n_consts][8]``."""
    base = np.ascontiguousarray(base, dtype=np.uint32).reshape(-1, 8)
    out = np.repeat(base[:, :, None], lanes, axis=2)
    for lane, row in enumerate(moves_ref(leafgen, consts, base, seed, r, lanes)):
        for leaf, _, v in row:
            out[leaf, :, lane] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    return out


@dataclass
class RepairResult:
    leaves: np.ndarray         # (n_leaves, 8) u32: the last base
    nfail: int                 # its failing constraints (0: a model of the program)
    rounds: int                # rounds run
    trace: np.ndarray          # (max_rounds,) the fewest failing constraints of each round run
    kernel_ms: float = 0.0     # device time of the rounds (not compared)


def repair_ref(bits_fn: Callable[[np.ndarray], np.ndarray], leafgen, consts, start, seed: int,
               lanes: int = 4096, max_rounds: int = 64, sync_every: int = 8) -> RepairResult:
    """The whole loop as ``mg_repair`` runs it.  ``bits_fn`` maps an SoA leaf
    array ``(n_leaves, 8, n)`` to ``(n, n_constraints)`` bool verdicts."""
    base = np.ascontiguousarray(start, dtype=np.uint32).reshape(-1, 8).copy()
    sync_every = sync_every or 8
    trace = np.zeros(max_rounds, dtype=np.uint32)
    base_nfail, r = None, 0
    while r < max_rounds and base_nfail != 0:
        stop = max_rounds if max_rounds - r < sync_every else r + sync_every
        while r < stop:
            nb = mutate_ref(leafgen, consts, base, seed, r, lanes)
            nfail = (~np.asarray(bits_fn(nb), dtype=bool)).sum(axis=1)
            lane = int(np.argmin(nfail))                  # the lowest lane of the minimum
            if base_nfail is None or int(nfail[lane]) < base_nfail:
                base, base_nfail = np.ascontiguousarray(nb[:, :, lane]), int(nfail[lane])
            trace[r] = int(nfail[lane])
            r += 1
    return RepairResult(base, base_nfail, r, trace)


# ---------------------------------------------------------------------------
# the scored walk: residual probes, the key, several walkers
# ---------------------------------------------------------------------------

# the constants of csrc/mg_walk.h
CW = 0x8CB92BA72F3D8DD7
FLAT, HAMMING, MAGNITUDE = range(3)
MAX_WALKERS = 64
RESIDUAL_BITS = 256

_LESS = ("bvult", "bvule", "bvslt", "bvsle")
_GREATER = ("bvugt", "bvuge", "bvsgt", "bvsge")


def _ite10(n) -> bool:
    return (n.op == "ite" and n.is_bv() and n.args[1].op == "bvnum" and n.args[2].op == "bvnum"
            and n.args[1].params[0] == 1 and n.args[2].params[0] == 0)


def peel(c):
    """``(d, negated)``: ``c`` is ``d`` or ``not d`` after dropping every
    ``not`` and LASER's Bool-as-word wrappers ``ite(d, 1, 0) = 0`` (``not
    d``) and ``ite(d, 1, 0) = 1`` (``d``)."""
    neg = False
    while True:
        if c.op == "not":
            c, neg = c.args[0], not neg
            continue
        if c.op == "=":
            a, b = c.args
            if _ite10(b):
                a, b = b, a
            if _ite10(a) and b.op == "bvnum" and b.params[0] in (0, 1):
                c, neg = a.args[0], neg != (b.params[0] == 0)
                continue
        return c, neg


def _difference(c):
    """``a - b`` of an order atom ``a < b`` / ``a <= b`` (``b - a`` of the
    ``>`` forms) over at most 256 bits, else None."""
    from .smt import node as N
    if c.op not in _LESS + _GREATER or c.args[0].width > RESIDUAL_BITS:
        return None
    a, b = c.args if c.op in _LESS else c.args[::-1]
    return N.bv_op("bvsub", a, b)


def classify(c):
    """``(kind, residual node or None)`` of one constraint."""
    from .smt import node as N
    c, neg = peel(c)
    if neg:
        return FLAT, None
    # (a one-bit equality's distance is identically 1: FLAT, and no probe)
    if c.op == "=" and c.args[0].is_bv() and 2 <= c.args[0].width <= RESIDUAL_BITS:
        return HAMMING, N.bv_op("bvxor", *c.args)
    atoms = [c] if c.op != "or" else [d for d, negated in map(peel, c.args) if not negated]
    for d in atoms:
        r = _difference(d)
        if r is not None:
            return MAGNITUDE, r
    return FLAT, None


def residuals(constraints: Sequence):
    """``(probes, table)``: the residual probe nodes of ``constraints`` (one
    per distinct term, to compile right after the mask probes) and ``table``
    (n_roots,) u32, ``kind << 16 | probe index``: what a failing root costs
    (``score_ref``).  The distance is a heuristic; whether a root holds is
    always read from its mask bit."""
    probes, index, table = [], {}, []
    for c in constraints:
        kind, r = classify(c)
        if r is None:
            table.append(FLAT << 16)
            continue
        if r.id not in index:
            index[r.id] = len(probes)
            probes.append(r)
        table.append(kind << 16 | index[r.id])
    return probes, np.array(table, dtype=np.uint32)


def flat_table(n_roots: int) -> np.ndarray:
    return np.zeros(n_roots, dtype=np.uint32)


def _score_bits(bits: np.ndarray, resid, table) -> tuple:
    """(nfail, cost) int64 (n,) of verdicts ``bits`` (n, n_roots) bool and
    residual values ``resid`` (n_resid, 8, n) u32."""
    fail = ~np.asarray(bits, dtype=bool)
    n, n_roots = fail.shape
    table = np.asarray(table, dtype=np.int64)
    kind, probe = table >> 16, table & 0xFFFF
    dist = np.ones((n, n_roots), dtype=np.int64)
    if (kind != FLAT).any():
        resid = np.ascontiguousarray(resid, dtype="<u4")
        pop = np.unpackbits(resid.view(np.uint8).reshape(resid.shape[0], 8, n, 4),
                            axis=3).sum(axis=(1, 3)).astype(np.int64)          # (n_resid, n)
        length = np.zeros(pop.shape, dtype=np.int64)
        for i in range(8):                               # the highest non-zero limb wins
            limb = resid[:, i, :]
            length = np.where(limb != 0, 32 * i + np.frexp(limb.astype(np.float64))[1], length)
        for k in np.flatnonzero(kind != FLAT):
            dist[:, k] = (np.maximum(1, pop[probe[k]]) if kind[k] == HAMMING
                          else 1 + length[probe[k]])
    return fail.sum(axis=1).astype(np.int64), (fail * dist).sum(axis=1).astype(np.int64)


def score_ref(masks: np.ndarray, resid, table, n_roots: int) -> tuple:
    """The key ``(nfail, cost)`` of every lane, from host mask probes
    ``masks`` (n_mask, 8, n) u32 and residual probes ``resid`` (n_resid, 8,
    n) u32 — the specification of ``csrc/mg_walk.h``.  A failing root k costs
    1 (FLAT), max(1, popcount(R_k)) (HAMMING) or 1 + bitlen(R_k)
    (MAGNITUDE); cost is the sum over the failing roots."""
    from .census import mask_bits
    return _score_bits(mask_bits(masks, n_roots), resid, table)


@dataclass
class WalkResult:
    leaves: np.ndarray         # (walkers, n_leaves, 8) u32: each walker's last base
    nfail: np.ndarray          # (walkers,) its failing constraints
    cost: np.ndarray           # (walkers,) and their summed distance
    rounds: int                # rounds run (every walker runs them all)
    trace: np.ndarray          # (walkers, max_rounds, 2) (nfail, cost) of each round's best
    winner: int                # the walker of minimum (nfail, cost, w)
    kernel_ms: float = 0.0     # device time of the rounds (not compared)


def walk_ref(values_fn: Callable, leafgen, consts, starts, table, seed: int, lanes: int = 4096,
             max_rounds: int = 64, sync_every: int = 8, score: Optional[Callable] = None,
             aims=None, bounds=None, ufs=None, sums=None) -> WalkResult:
    """The whole loop as ``mg_walk`` runs it.  ``values_fn`` maps an SoA leaf
    array ``(n_leaves, 8, n)`` to ``(bits (n, n_roots) bool, resid (n_resid,
    8, n) u32)``: the verdicts and the residual values.  Walker w moves under
    the seed ``seed ^ w * CW``; all walkers stop at the first sync after one
    of them has no failing root.

    ``score``: another scoring of the same loop (``mg_walk_tree``): called
    with what ``values_fn`` returns, it gives ``(nfail, cost)`` per lane, and
    ``table`` is not read (:func:`tree_scoring`).

    ``aims``: the aim table of ``mg_walk_aim`` (:func:`aim_table`): the
    neighbours are those of :func:`aim_mutate_ref` under the residual values
    of the walker's base — the last element of what ``values_fn`` returns, in
    the column of the lane it adopted (none before round 0's adoption).

    ``bounds``: the table of ``mg_walk_bound`` (:func:`bound_table`) instead:
    the neighbours are those of :func:`bound_mutate_ref` under the adopted
    lane's residual values, root bits (the first element of what ``values_fn``
    returns) and atom bits (the second of three; none without tree scoring).

    ``ufs``: with ``bounds``, the tables of ``mg_walk_uf`` (:func:`uf_table`):
    ``values_fn`` returns ``(bits, abits, resid, urows)``, the walker keeps the
    adopted lane's U rows ``urows[:, :, lane]`` and resolves its slots after
    each adoption (:func:`uf_resolve_ref` on the new base), and the neighbours
    are those of :func:`uf_mutate_ref`.

    ``sums``: with ``bounds`` and ``ufs``, the lin words of ``mg_walk_sum``
    (:func:`sum_table`): ``values_fn`` returns ``(bits, abits, resid, urows,
    srows)``, the walker also keeps the adopted lane's side rows ``srows[:, :,
    lane]``, and the neighbours are those of :func:`sum_mutate_ref`."""
    bases = np.ascontiguousarray(starts, dtype=np.uint32).copy()
    walkers = bases.shape[0]
    if not 1 <= walkers <= MAX_WALKERS or bases.shape[2:] != (8,):
        raise ValueError("starts must be (1..64 walkers, n_leaves, 8)")
    sync_every = sync_every or 8
    trace = np.zeros((walkers, max_rounds, 2), dtype=np.uint32)
    keys: List[Optional[tuple]] = [None] * walkers
    rvals: List[Optional[np.ndarray]] = [None] * walkers
    r = 0
    while r < max_rounds and not any(k is not None and k[0] == 0 for k in keys):
        stop = max_rounds if max_rounds - r < sync_every else r + sync_every
        while r < stop:
            if sums is not None:
                nb = np.concatenate([sum_mutate_ref(leafgen, consts, bases[w], rvals[w], bounds,
                                                    sums, seed ^ (w * CW & M64), r, lanes)
                                     for w in range(walkers)], axis=2)
            elif ufs is not None:
                nb = np.concatenate([uf_mutate_ref(leafgen, consts, bases[w], rvals[w], bounds,
                                                   seed ^ (w * CW & M64), r, lanes)
                                     for w in range(walkers)], axis=2)
            elif bounds is not None:
                nb = np.concatenate([bound_mutate_ref(leafgen, consts, bases[w], rvals[w], bounds,
                                                      seed ^ (w * CW & M64), r, lanes)
                                     for w in range(walkers)], axis=2)
            elif aims is None:
                nb = np.concatenate([mutate_ref(leafgen, consts, bases[w], seed ^ (w * CW & M64),
                                                r, lanes) for w in range(walkers)], axis=2)
            else:
                nb = np.concatenate([aim_mutate_ref(leafgen, consts, bases[w], rvals[w], aims,
                                                    seed ^ (w * CW & M64), r, lanes)
                                     for w in range(walkers)], axis=2)
            values = values_fn(nb)
            urows = srows = None
            if sums is not None:
                values, urows, srows = values[:3], values[3], values[4]
            elif ufs is not None:
                values, urows = values[:3], values[3]
            if score is None:
                nfail, cost = _score_bits(values[0], values[1], table)
            else:
                nfail, cost = score(*values)
            for w in range(walkers):
                nf, co = nfail[w * lanes:(w + 1) * lanes], cost[w * lanes:(w + 1) * lanes]
                lane = int(np.lexsort((co, nf))[0])       # stable: the lowest lane of the minimum
                key = (int(nf[lane]), int(co[lane]))
                if keys[w] is None or key < keys[w]:
                    bases[w], keys[w] = nb[:, :, w * lanes + lane], key
                    if bounds is not None:
                        at = w * lanes + lane
                        rvals[w] = (np.ascontiguousarray(values[-1][:, :, at]),
                                    np.array(values[0][at], dtype=bool),
                                    np.array(values[1][at] if len(values) == 3 else [],
                                             dtype=bool))
                        if ufs is not None:
                            rvals[w] += (uf_resolve_ref(bases[w], urows[:, :, at], ufs),)
                        if sums is not None:
                            rvals[w] += (np.ascontiguousarray(srows[:, :, at]),)
                    elif aims is not None:
                        rvals[w] = np.ascontiguousarray(values[-1][:, :, w * lanes + lane])
                trace[w, r] = key
            r += 1
    nfail = np.array([k[0] for k in keys], dtype=np.int64)
    cost = np.array([k[1] for k in keys], dtype=np.int64)
    winner = min(range(walkers), key=lambda w: (keys[w], w))
    return WalkResult(bases, nfail, cost, r, trace, winner)


# ---------------------------------------------------------------------------
# distance trees: branch distance through and, or, ite and
# store chains
# ---------------------------------------------------------------------------

# the constants of csrc/mg_walk_tree.h
WT_TREE = 1 << 31
WT_END, WT_ATOM, WT_AND, WT_OR, WT_PUSH_INF = range(5)
WT_INF = 1023
MAX_ATOMS, ROOT_ATOMS, ROOT_WORDS, ROOT_DEPTH, WT_STACK = 1024, 32, 64, 8, 8

_NEGATED_ORDER = {"bvult": "bvuge", "bvule": "bvugt", "bvugt": "bvule", "bvuge": "bvult",
                  "bvslt": "bvsge", "bvsle": "bvsgt", "bvsgt": "bvsle", "bvsge": "bvslt"}
_TRUE, _FALSE = ("true",), ("false",)


def _atom(node, pol: bool, kind: int = FLAT, resid=None):
    """An atom: the Boolean ``node`` (``not node`` when ``pol`` is False)
    holds, else it is ``kind``'s distance of ``resid`` away."""
    return ("atom", (node.id, pol), kind, node, pol, resid)


def _join(op: str, children):
    """AND / OR of trees, flattened, constants folded."""
    unit, zero = (_TRUE, _FALSE) if op == "and" else (_FALSE, _TRUE)
    out = []
    for c in children:
        if c == unit:
            continue
        if c == zero:
            return zero
        out.extend(c[1] if c[0] == op else [c])
    return unit if not out else out[0] if len(out) == 1 else (op, out)


def _measure(t):
    """(distinct atom keys, code words without END, stack, depth) of a tree
    as :func:`_emit` writes it (n children: n - 1 binary folds)."""
    if t[0] == "atom":
        return {t[1]}, 1, 1, 1
    if t[0] in ("true", "false"):
        return set(), 1, 1, 1
    keys, words, stack, depth = set(), len(t[1]) - 1, 0, 0
    for i, c in enumerate(t[1]):
        k, w, s, d = _measure(c)
        keys |= k
        words += w
        stack = max(stack, s + (1 if i else 0))
        depth = max(depth, d + 1)
    return keys, words, stack, depth


def _chunk(a, hi: int, lo: int):
    """``extract(hi, lo, a)`` with numerals and aligned concats simplified."""
    from .smt import node as N
    if lo == 0 and hi == a.width - 1:
        return a
    if a.op == "bvnum":
        return N.bv_num(a.params[0] >> lo, hi - lo + 1)
    if a.op == "concat":
        parts, top = [], a.width
        for arg in a.args:                               # high first
            base = top - arg.width
            if base <= hi and lo < top:
                parts.append(_chunk(arg, min(hi, top - 1) - base, max(lo, base) - base))
            top = base
        return N.concat(*parts)
    return N.extract(hi, lo, a)


class _TreeBuilder:
    """The rules of DESIGN.md §3.11 on one root."""

    def __init__(self):
        self.work = 0

    def flat(self, node, pol):
        return _atom(node, pol)

    def fits(self, t, level):
        keys, words, stack, depth = _measure(t)
        return (len(keys) <= ROOT_ATOMS and words + 1 <= ROOT_WORDS and stack <= WT_STACK
                and level - 1 + depth <= ROOT_DEPTH)

    def capped(self, t, level, node, pol):
        """``t``, or one FLAT atom of the subterm when its expansion exceeds
        the root's budget."""
        return t if self.fits(t, level) else self.flat(node, pol)

    def join(self, op, parts, level, node, pol):
        """AND / OR of the lazily built ``parts`` (callables of a level); a
        node that outgrows the budget while it is built collapses at once."""
        out = []
        for p in parts:
            out.append(p(level + 1))
            if sum(len(_measure(c)[0]) for c in out) > 4 * ROOT_ATOMS:
                return self.flat(node, pol)
        return self.capped(_join(op, out), level, node, pol)

    def boolean(self, c, pol: bool, level: int):
        """The tree of ``c`` (``not c`` when ``pol`` is False)."""
        from .smt import node as N
        c, neg = peel(c)
        pol = pol != neg
        op = c.op
        if op in ("true", "false"):
            return _TRUE if (op == "true") == pol else _FALSE
        if level > ROOT_DEPTH:
            return self.flat(c, pol)
        if op in ("and", "or"):
            kind = op if pol else ("or" if op == "and" else "and")       # De Morgan
            return self.join(kind, [lambda lv, a=a: self.boolean(a, pol, lv) for a in c.args],
                             level, c, pol)
        if op == "=>":
            a, b = c.args
            return self.join("or" if pol else "and",
                             [lambda lv: self.boolean(a, not pol, lv),
                              lambda lv: self.boolean(b, pol, lv)], level, c, pol)
        if op == "ite" and c.is_bool():
            g, x, y = c.args
            arm = lambda cond, v: lambda lv: self.join(
                "and", [lambda l2: self.boolean(g, cond, l2), lambda l2: self.boolean(v, pol, l2)],
                lv, c, pol)
            return self.join("or", [arm(True, x), arm(False, y)], level, c, pol)
        if op == "=" and c.args[0].is_bv():
            return self.equality(c.args[0], c.args[1], pol, level)
        if op in _NEGATED_ORDER:
            if not pol:                                  # not (a < b): b <= a
                c = N.bv_cmp(_NEGATED_ORDER[op], *c.args)
            r = _difference(c)
            return self.flat(c, True) if r is None else _atom(c, True, MAGNITUDE, r)
        return self.flat(c, pol)                         # Bool xor, Bool =, distinct, a variable ..

    def cases(self, a):
        """``[(conditions, value)]`` when ``a`` is a bit-vector ite or a read
        of a store chain: ``a`` is ``value`` where every ``(Bool node,
        polarity)`` of ``conditions`` holds; else None.  A chain is one flat
        case split: key k hits and the keys above it miss."""
        from .smt import node as N
        if a.op == "ite":
            g, x, y = a.args
            return [([(g, True)], x), ([(g, False)], y)]
        if a.op != "select" or a.args[0].op not in ("store", "K"):
            return None
        arr, j = a.args
        out, missed = [], []
        while arr.op == "store":
            below, i, v = arr.args
            hit = N.eq(i, j)
            out.append((missed + [(hit, True)], v))
            missed = missed + [(hit, False)]
            arr = below
        out.append((missed, arr.args[0] if arr.op == "K" else N.select(arr, j)))
        return out

    def equality(self, a, b, pol: bool, level: int):
        """``a = b`` (``a != b`` when ``pol`` is False) of bit-vectors."""
        from .smt import node as N
        whole = N.eq(a, b)
        self.work += 1
        if a.op == "bvnum" and b.op == "bvnum":
            return _TRUE if (a.params[0] == b.params[0]) == pol else _FALSE
        if level > ROOT_DEPTH or self.work > 4096:
            return self.flat(whole, pol)
        for x, y in ((a, b), (b, a)):
            split = self.cases(x)
            if split is None:
                continue
            arm = lambda conds, v: lambda lv: self.join(
                "and", [lambda l2, g=g, p=p: self.boolean(g, p, l2) for g, p in conds]
                + [lambda l2: self.equality(v, y, pol, l2)], lv, whole, pol)
            return self.join("or", [arm(conds, v) for conds, v in split], level, whole, pol)
        if not pol:
            return self.flat(whole, False)               # an inequality has no distance
        if a.op == "apply" and b.op == "apply" and a.params == b.params:     # congruence
            return self.join("or", [lambda lv: self.equality(a.args[0], b.args[0], True, lv),
                                    lambda lv: self.distance(a, b, lv)], level, whole, True)
        return self.distance(a, b, level)

    def distance(self, a, b, level: int):
        """Positive ``a = b`` with no case split left."""
        from .smt import node as N
        w = a.width
        if w > RESIDUAL_BITS:                            # extract first, then xor
            parts = [lambda lv, lo=lo: self.equality(_chunk(a, min(lo + RESIDUAL_BITS, w) - 1, lo),
                                                     _chunk(b, min(lo + RESIDUAL_BITS, w) - 1, lo),
                                                     True, lv)
                     for lo in range(0, w, RESIDUAL_BITS)]
            return self.join("and", parts, level, N.eq(a, b), True)
        if a.op == "bvnum" and b.op == "bvnum":
            return _TRUE if a.params[0] == b.params[0] else _FALSE
        if w == 1:
            return self.flat(N.eq(a, b), True)
        return _atom(N.eq(a, b), True, HAMMING, N.bv_op("bvxor", a, b))


@dataclass
class Trees:
    """The tables of ``mg_walk_tree`` (``csrc/mg_walk_tree.h``) for a list of
    constraints: probe order ``[root mask | atom mask | residuals]``."""
    roots: np.ndarray          # (n_roots,) u32: kind << 16 | probe, or WT_TREE | offset in code
    atoms: np.ndarray          # (n_atoms,) u32: kind << 16 | residual probe
    code: np.ndarray           # (n_code,) u32: op << 16 | argument, postfix
    atom_nodes: list           # the Bool node of every atom's truth bit (census.mask_probes)
    probes: list               # the residual probe nodes, one per distinct term
    shapes: list               # per root its tree: ("atom", index) | ("and" | "or", [..]) | ("false",)

    @property
    def n_atoms(self) -> int:
        return len(self.atoms)

    @property
    def n_resid(self) -> int:
        return len(self.probes)

    def is_tree(self, k: int) -> bool:
        return bool(int(self.roots[k]) & WT_TREE)

    def kind(self, k: int) -> int:
        """A simple root's kind."""
        return int(self.roots[k]) >> 16

    def listing(self, k: int, depth: int = 3, state=None) -> str:
        """Root ``k``'s tree, indented, every atom with its kind and its
        s-expression to ``depth``; ``state``: per atom (holds, distance) on
        some assignment, shown with each atom."""
        from .smt import node as N
        names = ("FLAT", "HAMMING", "MAGNITUDE")
        lines = []

        def walk(t, ind):
            if t[0] == "atom":
                e = int(self.atoms[t[1]])
                now = "" if state is None else (
                    " [holds]" if state[t[1]][0] else " [%d away]" % state[t[1]][1])
                lines.append("%satom %d %s%s %s" % ("  " * ind, t[1], names[e >> 16], now,
                                                     N.to_sexpr(self.atom_nodes[t[1]], depth)))
            elif t[0] in ("and", "or"):
                lines.append("  " * ind + t[0].upper())
                for c in t[1]:
                    walk(c, ind + 1)
            else:
                lines.append("  " * ind + t[0].upper())
        walk(self.shapes[k], 0)
        return "\n".join(lines)


def simple_trees(table) -> Trees:
    """A residual table of :func:`residuals` as all-simple ``Trees``."""
    table = np.ascontiguousarray(table, dtype=np.uint32)
    return Trees(table, np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), [], [],
                 [("simple",)] * len(table))


def distance_trees(constraints: Sequence) -> Trees:
    """The distance trees of ``constraints``.  A root's cost
    when it fails is the branch distance of its Boolean structure: AND = sum,
    OR = minimum, negation pushed to the atoms, bit-vector ``ite`` and reads
    of store chains as case splits, UF congruence as one more OR arm; atoms
    are the three kinds of :func:`residuals`.  A root that is one atom is a
    simple entry, exactly a :func:`residuals` table entry (but a negated order
    is the opposite order, ``MAGNITUDE``).  Atoms are shared across roots by
    (node, polarity), residual probes by term; past ``MAX_ATOMS`` atoms the
    remaining roots stay simple (:func:`classify`)."""
    from .smt import node as N
    probes, pindex = [], {}
    atom_nodes, atoms, aindex = [], [], {}
    roots, code, shapes = [], [], []

    def entry(kind, resid):
        if resid is None or kind == FLAT:
            return FLAT << 16
        if resid.id not in pindex:
            pindex[resid.id] = len(probes)
            probes.append(resid)
        return kind << 16 | pindex[resid.id]

    def emit(t):
        if t[0] == "atom":
            _, key, kind, node, pol, resid = t
            if key not in aindex:
                aindex[key] = len(atoms)
                atoms.append(entry(kind, resid))
                atom_nodes.append(node if pol else N.bool_op("not", node))
            code.append(WT_ATOM << 16 | aindex[key])
            return ("atom", aindex[key])
        if t[0] == "false":
            code.append(WT_PUSH_INF << 16)
            return ("false",)
        op = WT_AND if t[0] == "and" else WT_OR
        kids = []
        for i, c in enumerate(t[1]):
            kids.append(emit(c))
            if i:
                code.append(op << 16 | 2)
        return (t[0], kids)

    for c in constraints:
        t = _TreeBuilder().boolean(c, True, 1)
        if t[0] in ("and", "or") and len(aindex) + len(_measure(t)[0] - set(aindex)) > MAX_ATOMS:
            kind, r = classify(c)
            roots.append(entry(kind, r))
            shapes.append(("simple",))
        elif t[0] in ("and", "or"):
            roots.append(WT_TREE | len(code))
            shapes.append(emit(t))
            code.append(WT_END << 16)
        else:                                            # one atom, or a constant
            roots.append(entry(t[2], t[5]) if t[0] == "atom" else FLAT << 16)
            shapes.append(("simple",))
    return Trees(np.array(roots, dtype=np.uint32), np.array(atoms, dtype=np.uint32),
                 np.array(code, dtype=np.uint32), atom_nodes, probes, shapes)


def _distances(resid: np.ndarray, n: int):
    """(popcount, bit length) (n_resid, n) int64 of residual values."""
    resid = np.ascontiguousarray(resid, dtype="<u4")
    pop = np.unpackbits(resid.view(np.uint8).reshape(resid.shape[0], 8, n, 4),
                        axis=3).sum(axis=(1, 3)).astype(np.int64)
    length = np.zeros(pop.shape, dtype=np.int64)
    for i in range(8):
        limb = resid[:, i, :]
        length = np.where(limb != 0, 32 * i + np.frexp(limb.astype(np.float64))[1], length)
    return pop, length


def _tree_score_bits(bits, abits, resid, trees: Trees) -> tuple:
    """(nfail, cost) int64 (n,) of root verdicts ``bits`` (n, n_roots) bool,
    atom verdicts ``abits`` (n, n_atoms) bool and residual values."""
    fail = ~np.asarray(bits, dtype=bool)
    n, n_roots = fail.shape
    pop = length = None
    if resid is not None and len(resid):
        pop, length = _distances(resid, n)

    def dist(e):
        kind, p = int(e) >> 16, int(e) & 0xFFFF
        return (np.ones(n, dtype=np.int64) if kind == FLAT else
                np.maximum(1, pop[p]) if kind == HAMMING else 1 + length[p])

    cost = np.zeros(n, dtype=np.int64)
    for k in np.flatnonzero(fail.any(axis=0)):
        e = int(trees.roots[k])
        if not e & WT_TREE:
            cost += fail[:, k] * dist(e)
            continue
        stack, pc = [], e & ~WT_TREE
        while True:
            op, arg = int(trees.code[pc]) >> 16, int(trees.code[pc]) & 0xFFFF
            pc += 1
            if op == WT_END:
                break
            if op == WT_ATOM:
                stack.append(np.where(abits[:, arg], 0, dist(trees.atoms[arg])))
            elif op == WT_PUSH_INF:
                stack.append(np.full(n, WT_INF, dtype=np.int64))
            else:
                args = stack[len(stack) - arg:]
                del stack[len(stack) - arg:]
                stack.append(np.minimum(WT_INF, np.sum(args, axis=0)) if op == WT_AND
                             else np.min(args, axis=0))
        cost += fail[:, k] * np.clip(stack[0], 1, WT_INF)
    return fail.sum(axis=1).astype(np.int64), cost


def tree_score_ref(masks: np.ndarray, amasks, resid, trees: Trees, n_roots: int) -> tuple:
    """The key ``(nfail, cost)`` of every lane from host root-mask probes
    ``masks``, atom-mask probes ``amasks`` (n_amask, 8, n) u32 and residual
    probes ``resid`` — the specification of ``csrc/mg_walk_tree.h``.  A
    failing simple root costs what :func:`score_ref` says; a failing tree root
    ``clamp(value of its program, 1, 1023)``: ``ATOM i`` is 0 where atom i's
    bit is set, else its distance; ``AND`` the sum saturating at 1023, ``OR``
    the minimum, ``INF`` 1023."""
    from .census import mask_bits
    bits = mask_bits(masks, n_roots)
    abits = (mask_bits(amasks, trees.n_atoms) if trees.n_atoms
             else np.zeros((bits.shape[0], 0), dtype=bool))
    return _tree_score_bits(bits, abits, resid, trees)


def tree_scoring(trees: Trees) -> Callable:
    """The ``score`` argument of :func:`walk_ref` for ``trees``: its
    ``values_fn`` then returns ``(bits, abits, resid)``."""
    return lambda bits, abits, resid: _tree_score_bits(bits, abits, resid, trees)


# ---------------------------------------------------------------------------
# aimed moves: a failing equality's residual says which bits
# of which leaves to flip
# ---------------------------------------------------------------------------

# the constants of csrc/mg_walk_aim.h
AIM_MAX_ENTRIES, AIM_MAX_PIECES, AIM_NONE = 256, 64, 0xFFFFFFFF


@dataclass
class Aims:
    """The aim table of ``mg_walk_aim`` (``csrc/mg_walk_aim.h``)."""
    entries: np.ndarray        # (n_entries, 3) u32: residual probe, first piece, pieces
    pieces: np.ndarray         # (n_pieces, 4) u32: leaf, leaf_bit, value_bit, len
    sides: list                # per entry: which side of its probe's xor it moves (0: a, 1: b)

    def __len__(self) -> int:
        return len(self.entries)

    def of(self, e: int) -> list:
        """Entry ``e``'s pieces as (leaf, leaf_bit, value_bit, len) tuples."""
        _, off, cnt = (int(x) for x in self.entries[e])
        return [tuple(int(x) for x in row) for row in self.pieces[off:off + cnt]]


def no_aims() -> Aims:
    return Aims(np.zeros((0, 3), dtype=np.uint32), np.zeros((0, 4), dtype=np.uint32), [])


def make_aims(entries) -> Aims:
    """``Aims`` of ``[(residual probe, [(leaf, leaf_bit, value_bit, len), ..]), ..]``."""
    rows, pieces = [], []
    for p, ps in entries:
        rows.append((p, len(pieces), len(ps)))
        pieces.extend(ps)
    return Aims(np.array(rows, dtype=np.uint32).reshape(-1, 3),
                np.array(pieces, dtype=np.uint32).reshape(-1, 4), [0] * len(rows))


def _fold_key(i, subst) -> Optional[int]:
    """The value of a read's index when it is a numeral, a node the presets
    replace by one, or a sum of such; else None."""
    if i.op == "bvnum":
        return i.params[0]
    if i.id in subst:
        return subst[i.id] % (1 << i.width)
    if i.op == "bvadd":
        parts = [_fold_key(a, subst) for a in i.args]
        return None if None in parts else sum(parts) % (1 << i.width)
    return None


def aim_pieces(t, program, _slots=None, _rules: bool = False) -> Optional[list]:
    """The pieces ``[(leaf, leaf_bit, value_bit, len)]`` of the bit-vector
    term ``t`` as a destination, ``value_bit`` relative to
    ``t``'s bit 0; None when ``t`` does not resolve.  A numeral resolves to no
    piece.  ``_rules``: with the mask and shift rules of §3.15
    (:func:`sum_table` alone passes it)."""
    side = _resolve_side(t, program, _slots, _rules)
    return None if side is None else side[0]


def _pow2(v: int) -> Optional[int]:
    """c when v == 2^c, else None."""
    return v.bit_length() - 1 if v > 0 and v & (v - 1) == 0 else None


def _shift_of(t) -> Optional[tuple]:
    """``(operand, c, left)`` when ``t`` is a shift of one operand by the
    numeral c: ``bvlshr(x, c)``, ``bvudiv(x, 2^c)``,
    ``bvshl(x, c)`` or a ``bvmul`` of one non-numeral operand and numerals
    whose product is 2^c; else None."""
    if t.op in ("bvlshr", "bvshl") and t.args[1].op == "bvnum" and t.args[0].op != "bvnum":
        return t.args[0], t.args[1].params[0], t.op == "bvshl"
    if t.op == "bvudiv" and t.args[1].op == "bvnum" and t.args[0].op != "bvnum":
        c = _pow2(t.args[1].params[0])
        return None if c is None else (t.args[0], c, False)
    if t.op == "bvmul":
        rest = [a for a in t.args if a.op != "bvnum"]
        prod = 1
        for a in t.args:
            if a.op == "bvnum":
                prod *= a.params[0]
        c = _pow2(prod)
        return None if len(rest) != 1 or c is None else (rest[0], c, True)
    return None


def _mask_of(t) -> Optional[tuple]:
    """``(operand, keep, ones)`` when ``t`` is ``bvand`` / ``bvor`` of exactly
    one non-numeral operand and numerals: the bits of the operand that pass
    (``keep``) and the bits that are fixed ones; else None."""
    if t.op not in ("bvand", "bvor"):
        return None
    rest = [a for a in t.args if a.op != "bvnum"]
    if len(rest) != 1 or len(rest) == len(t.args):
        return None
    full = (1 << t.width) - 1
    m = full if t.op == "bvand" else 0
    for a in t.args:
        if a.op == "bvnum":
            m = m & a.params[0] if t.op == "bvand" else m | a.params[0]
    m &= full
    return (rest[0], m, 0) if t.op == "bvand" else (rest[0], full & ~m, m)


def _cut_pieces(pieces, keep: int) -> list:
    """``pieces`` cut to the runs of set bits of ``keep`` (value bits)."""
    out = []
    for l, lb, vb, n in pieces:
        b = vb
        while b < vb + n:
            if not keep >> b & 1:
                b += 1
                continue
            e = b
            while e < vb + n and keep >> e & 1:
                e += 1
            out.append((l, lb + b - vb, b, e - b))
            b = e
    return out


def _resolve_side(t, program, slots=None, rules: bool = False) -> Optional[tuple]:
    """``(pieces, fixed)`` of ``t`` by the rules of :func:`aim_pieces`;
    ``fixed``: the bits of ``t`` that numerals give (a numeral, or a numeral
    operand of a concat, at its offset; the numeral arm of an ``ite`` gives
    none), as an int.  ``slots`` ({apply node id: slot}, :func:`uf_table`
    alone passes it): an application with a slot u is the one piece ``(UF_SLOT
    | u, 0, 0, width)``, and one at a numeral argument that is a constant key
    of its function is that entry's ``cval`` leaf.  ``rules`` (DESIGN.md
    §3.15): ``bvand`` / ``bvor`` with numerals cut the pieces of their one
    other operand to the runs of passing bits (the rest is fixed 0, or 1), a
    right shift by a numeral (``bvlshr``, ``bvudiv`` by 2^c) is ``extract(w -
    1, c, .)`` zero-extended and a left shift (``bvshl``, ``bvmul`` by 2^c)
    ``concat(extract(w - 1 - c, 0, .), 0_c)``."""
    leaves = {(l.kind, l.source, l.entry, l.chunk): i for i, l in enumerate(program.leaves)}
    subst = getattr(program.presets, "subst", None) or {}

    def cells(kind, source, entry, width):
        out = []
        for k in range((width + RESIDUAL_BITS - 1) // RESIDUAL_BITS):
            li = leaves.get((kind, source, entry, k))
            if li is None or program.leaves[li].width != min(RESIDUAL_BITS,
                                                             width - RESIDUAL_BITS * k):
                return None
            out.append((li, 0, RESIDUAL_BITS * k, program.leaves[li].width))
        return out

    def leafy(ps):
        return None if ps is None else (ps, 0)

    def go(t):
        if t.op == "bvnum":
            return [], t.params[0] % (1 << t.width)
        if t.op == "var" and t.is_bv():
            return leafy(cells("var", t.params[0], 0, t.width))
        if t.op == "concat":
            out, fixed, off = [], 0, t.width
            for a in t.args:                             # high first
                off -= a.width
                side = go(a)
                if side is None:
                    return None
                out += [(l, lb, vb + off, n) for l, lb, vb, n in side[0]]
                fixed |= side[1] << off
            return out, fixed
        if t.op == "extract":
            hi, lo = t.params
            side = go(t.args[0])
            if side is None:
                return None
            out = []
            for l, lb, vb, n in side[0]:
                s, e = max(vb, lo), min(vb + n, hi + 1)
                if s < e:
                    out.append((l, lb + s - vb, s - lo, e - s))
            return out, side[1] >> lo & ((1 << (hi - lo + 1)) - 1)
        if t.op == "zero_extend":
            return go(t.args[0])
        if t.op == "ite" and t.is_bv():                  # the guard is ignored: a proposal
            _, x, y = t.args
            if x.op == "bvnum" or y.op == "bvnum":
                side = go(y if x.op == "bvnum" else x)
                # (an arm that is itself a numeral: no piece, and no fixed bit)
                return side if side is None or side[0] else ([], 0)
            return None
        if t.op == "select" and t.args[0].op == "array":
            name = t.args[0].params[0]
            key = _fold_key(t.args[1], subst)
            ckeys = list(program.table_ckeys.get(name, []))
            if key is None or key not in ckeys:
                return None
            return leafy(cells("cval", name, ckeys.index(key), t.width))
        if t.op == "apply" and slots is not None:
            if t.id in slots:
                return [(UF_SLOT | slots[t.id], 0, 0, t.width)], 0
            name, key = t.params[0], _fold_key(t.args[0], subst)
            ckeys = list(program.table_ckeys.get(name, []))
            if key is None or key not in ckeys:
                return None
            return leafy(cells("cval", name, ckeys.index(key), t.width))
        if rules and _mask_of(t) is not None:
            x, keep, ones = _mask_of(t)
            side = go(x)
            if side is None:
                return None
            return _cut_pieces(side[0], keep), side[1] & keep | ones
        if rules and _shift_of(t) is not None:
            x, c, left = _shift_of(t)
            side = go(x)
            if side is None:
                return None
            w = t.width
            if c >= w:
                return [], 0
            if left:                                     # bits 0 .. w - 1 - c move up by c
                return ([(l, lb, vb + c, n) for l, lb, vb, n in
                         _cut_pieces(side[0], (1 << (w - c)) - 1)],
                        side[1] << c & ((1 << w) - 1))
            return ([(l, lb, vb - c, n) for l, lb, vb, n in
                     _cut_pieces(side[0], ((1 << w) - 1) & ~((1 << c) - 1))], side[1] >> c)
        return None
    return go(t)


def aim_refusal(t, program, ufs=None, rules: bool = False) -> Optional[str]:
    """Why :func:`aim_pieces` does not resolve ``t`` (the first subterm no
    rule takes, with the rule that refused it), None when it resolves.
    ``ufs``: the tables of :func:`uf_table`; an ``apply`` then resolves where
    it has a slot, and else the reason says why it got none.  ``rules``: with
    the mask and shift rules of §3.15; a mask or shift those rules do not take
    says which operand stands in the way."""
    slots = None if ufs is None else ufs.slot_of
    if aim_pieces(t, program, slots, rules) is not None:
        return None
    if t.op in ("concat", "extract", "zero_extend"):
        return next((r for r in (aim_refusal(a, program, ufs, rules) for a in t.args) if r),
                    "%s over a sum: only the top of a side is flattened" % t.op)
    if t.op == "ite" and t.is_bv():
        _, x, y = t.args
        if x.op == "bvnum" or y.op == "bvnum":
            return aim_refusal(y if x.op == "bvnum" else x, program, ufs, rules)
        return "ite: neither arm is a numeral"
    if rules and t.op in ("bvand", "bvor"):
        got = _mask_of(t)
        if got is None:
            return "%s: not one operand and numerals" % t.op
        return aim_refusal(got[0], program, ufs, rules)
    if rules and t.op in ("bvlshr", "bvshl", "bvudiv", "bvmul"):
        got = _shift_of(t)
        if got is None:
            return "%s: not one operand and %s" % (
                t.op, "a numeral shift" if t.op in ("bvlshr", "bvshl") else "a numeral 2^c")
        return aim_refusal(got[0], program, ufs, rules)
    if rules and t.op in ("bvadd", "bvsub", "bvneg"):
        terms = linear_terms(t)
        if terms is None:
            return "%s: more than %d terms, or wider than %d bits" % (t.op, SUM_MAX_TERMS,
                                                                     RESIDUAL_BITS)
        why = [sum_target(t, i, program) for i in range(len(terms))]
        if all(isinstance(w, str) for w in why):
            return "%s: no eligible target (%s)" % (t.op, "; ".join(dict.fromkeys(why)))
        return None
    if t.op == "apply" and ufs is not None:
        name = t.params[0]
        if t.width > RESIDUAL_BITS:
            return "apply(%s): the range (%d bits) is wider than %d" % (name, t.width,
                                                                        RESIDUAL_BITS)
        if t.params[1] > RESIDUAL_BITS * UF_MAX_CHUNKS:
            return "apply(%s): the domain (%d bits) is wider than %d" % (
                name, t.params[1], RESIDUAL_BITS * UF_MAX_CHUNKS)
        if t.args[0].op == "bvnum":
            return "apply(%s, %d): the program does not read that constant key" % (
                name, t.args[0].params[0])
        if t.id in ufs.underived:
            return "apply(%s): every candidate's value is a derived leaf" % name
        return "apply(%s): over the cap of %d slots, %d candidates or %d U rows" % (
            name, UF_MAX_SLOTS, UF_MAX_CANDS, UF_MAX_ROWS)
    if t.op == "var":
        return "variable %s is not a leaf of the program" % t.params[0]
    if t.op == "select" and t.args[0].op == "array":
        name = t.args[0].params[0]
        key = _fold_key(t.args[1], getattr(program.presets, "subst", None) or {})
        if key is None:
            return "select(%s, .): the key (%s) is not a numeral under the presets" % (
                name, t.args[1].op)
        return "select(%s, %d): the program does not read that constant key" % (name, key)
    if t.op == "select":
        return "select of a %s" % t.args[0].op
    return "%s is not a destination" % t.op


def aim_table(trees: Trees, program, _slots=None) -> Aims:
    """The aim table of ``trees`` on the compiled ``program`` (DESIGN.md
    §3.12): for every residual probe ``bvxor(a, b)`` that a HAMMING atom or a
    simple HAMMING root of ``trees`` reads, in probe order, one entry per side
    (``a``, then ``b``) that :func:`aim_pieces` resolves to 1 .. 64 pieces
    none of whose leaves the program derives; at most 256 entries, the first
    ones."""
    used = set()
    for e in list(trees.atoms) + [r for r in trees.roots if not int(r) & WT_TREE]:
        if int(e) >> 16 == HAMMING:
            used.add(int(e) & 0xFFFF)
    rows, pieces, sides = [], [], []
    for p in sorted(used):
        node = trees.probes[p]
        if node.op != "bvxor" or len(node.args) != 2:
            continue
        for side, t in enumerate(node.args):
            ps = aim_pieces(t, program, _slots)
            if not ps or len(ps) > AIM_MAX_PIECES or any(l in program.derived for l, *_ in ps):
                continue
            if len(rows) < AIM_MAX_ENTRIES:
                rows.append((p, len(pieces), len(ps)))
                pieces.extend(ps)
                sides.append(side)
    return Aims(np.array(rows, dtype=np.uint32).reshape(-1, 3),
                np.array(pieces, dtype=np.uint32).reshape(-1, 4), sides)


def aim_picks_ref(rvals, aims: Aims, r: int, lanes: int) -> np.ndarray:
    """(lanes,) int64: the entry lane j of round ``r`` applies under the base's
    residual values ``rvals`` ((n_resid, 8) u32, None in round 0), or
    ``AIM_NONE``.  L = the entries whose residual is not zero, in table order,
    n1 = min(|L|, lanes // 8): lanes 1 .. n1 and n1 + 1 .. 2 n1 take
    L[(j' - 1 + r n1) mod |L|], j' = j or j - n1."""
    out = np.full(lanes, AIM_NONE, dtype=np.int64)
    if rvals is None or not len(aims):
        return out
    rv = np.asarray(rvals, dtype=np.uint32).reshape(-1, 8)
    live = [e for e in range(len(aims)) if rv[int(aims.entries[e, 0])].any()]
    n1 = min(len(live), lanes // 8)
    for j in range(1, 2 * n1 + 1):
        out[j] = live[((j if j <= n1 else j - n1) - 1 + r * n1) % len(live)]
    return out


def aim_mutate_ref(leafgen, consts, base, rvals, aims: Aims, seed: int, r: int,
                   lanes: int) -> np.ndarray:
    """``[n_leaves][8][lanes]`` u32: the neighbours of ``base`` that round
    ``r`` of ``mg_walk_aim`` evaluates — the specification of
    ``csrc/mg_walk_aim.h``.  Lane 0 is the base; a lane with an entry
    (:func:`aim_picks_ref`) has every piece of it applied to the base, ``leaf
    ^= ((R >> value_bit) & mask(len)) << leaf_bit`` with R the entry's
    residual value; the first n1 of them are that and nothing else, the next
    n1 then take the moves of :func:`moves_ref` for their lane, computed from
    the base and written over the aimed result; every other lane is
    :func:`mutate_ref`'s."""
    base = np.ascontiguousarray(base, dtype=np.uint32).reshape(-1, 8)
    picks = aim_picks_ref(rvals, aims, r, lanes)
    n1 = int((picks != AIM_NONE).sum()) // 2
    out = np.repeat(base[:, :, None], lanes, axis=2)
    moves = moves_ref(leafgen, consts, base, seed, r, lanes)
    bvals = _ints(base)
    rv = _ints(np.asarray(rvals, dtype=np.uint32).reshape(-1, 8)) if n1 else []
    for lane in range(lanes):
        cur = {}
        if picks[lane] != AIM_NONE:
            e = int(picks[lane])
            R = rv[int(aims.entries[e, 0])]
            for leaf, leaf_bit, value_bit, n in aims.of(e):
                cur[leaf] = cur.get(leaf, bvals[leaf]) ^ ((R >> value_bit & ((1 << n) - 1)) << leaf_bit)
        if lane > n1:
            for leaf, _, v in moves[lane]:
                cur[leaf] = v
        for leaf, v in cur.items():
            out[leaf, :, lane] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    return out


# ---------------------------------------------------------------------------
# aims for orders: a failing order's difference says what
# value one of its sides must take
# ---------------------------------------------------------------------------

# the constants of csrc/mg_walk_bound.h
BOUND_XOR, BOUND_LOW, BOUND_LOW_STRICT, BOUND_HIGH, BOUND_HIGH_STRICT = range(5)
BOUND_ATOM = 1 << 31
_STRICT = ("bvult", "bvslt", "bvugt", "bvsgt")
M256 = (1 << 256) - 1


@dataclass
class Bounds:
    """The table of ``mg_walk_bound`` (``csrc/mg_walk_bound.h``)."""
    entries: np.ndarray        # (n, 5) u32: residual probe, first piece, pieces, mode, truth
    pieces: np.ndarray         # (m, 4) u32: leaf, leaf_bit, value_bit, len
    fixed: np.ndarray          # (n, 8) u32: the numeral bits of an order entry's side
    sides: list                # per entry: XOR: the side of the xor it moves; order: 0 lo, 1 hi
    n_roots: int = 0           # what the truth indices are below
    n_atoms: int = 0

    def __len__(self) -> int:
        return len(self.entries)

    @property
    def n_order(self) -> int:
        return int((self.entries[:, 3] != BOUND_XOR).sum()) if len(self.entries) else 0

    def of(self, e: int) -> list:
        """Entry ``e``'s pieces as (leaf, leaf_bit, value_bit, len) tuples."""
        _, off, cnt = (int(x) for x in self.entries[e, :3])
        return [tuple(int(x) for x in row) for row in self.pieces[off:off + cnt]]

    def fixed_of(self, e: int) -> int:
        return _ints(self.fixed[e:e + 1])[0]


def _u256(v: int) -> np.ndarray:
    return np.frombuffer((v & M256).to_bytes(32, "little"), dtype="<u4")


def make_bounds(entries, n_roots: int = 0, n_atoms: int = 0) -> Bounds:
    """``Bounds`` of ``[(residual probe, pieces, mode, truth, fixed int), ..]``
    (an aim-table pair ``(probe, pieces)`` is an XOR entry)."""
    rows, pieces, fixed, sides = [], [], [], []
    for ent in entries:
        p, ps, mode, truth, fx = tuple(ent) + (BOUND_XOR, 0, 0)[len(ent) - 2:]
        rows.append((p, len(pieces), len(ps), mode, truth))
        pieces.extend(ps)
        fixed.append(_u256(fx))
        sides.append(1 if mode >= BOUND_HIGH else 0)
    return Bounds(np.array(rows, dtype=np.uint32).reshape(-1, 5),
                  np.array(pieces, dtype=np.uint32).reshape(-1, 4),
                  np.array(fixed, dtype=np.uint32).reshape(-1, 8), sides, n_roots, n_atoms)


def bounds_of_aims(aims: Aims, n_roots: int = 0, n_atoms: int = 0) -> Bounds:
    """An aim table as XOR entries."""
    n = len(aims)
    entries = np.zeros((n, 5), dtype=np.uint32)
    entries[:, :3] = aims.entries
    return Bounds(entries, np.array(aims.pieces, dtype=np.uint32).reshape(-1, 4),
                  np.zeros((n, 8), dtype=np.uint32), list(aims.sides), n_roots, n_atoms)


def bound_mask_words(bits) -> np.ndarray:
    """Mask bits as the words of their mask probes' rows (``census.mask_probes``:
    bit k is bit k % 32 of word k / 32), ``ceil(n / 256) * 8`` u32."""
    bits = np.asarray(bits, dtype=bool)
    out = np.zeros((len(bits) + 255) // 256 * 256, dtype=bool)
    out[:len(bits)] = bits
    return np.packbits(out.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)


def order_sides(node, negated: bool = False):
    """``(lo, hi, strict)`` of an order atom (of the opposite order when
    ``negated``), oriented as :func:`_difference` orients it (its residual is
    ``lo - hi``), or None."""
    if node.op not in _LESS + _GREATER:
        return None
    op = _NEGATED_ORDER[node.op] if negated else node.op
    lo, hi = node.args if op in _LESS else node.args[::-1]
    return lo, hi, op in _STRICT


def _order_probe(trees: Trees, lo, hi) -> Optional[int]:
    """The ``bvsub(lo, hi)`` among ``trees.probes``, by its operands' ids."""
    for p, d in enumerate(trees.probes):
        if d.op == "bvsub" and len(d.args) == 2 and (d.args[0].id, d.args[1].id) == (lo.id, hi.id):
            return p
    return None


def bound_side(t, program, _slots=None) -> Optional[tuple]:
    """``(pieces, fixed)`` of one side of an order as a destination (DESIGN.md
    §3.13), or None: the side does not resolve, has no piece or more than 64,
    or one of its leaves is derived by the program."""
    side = _resolve_side(t, program, _slots)
    if side is None or not side[0] or len(side[0]) > AIM_MAX_PIECES or \
            any(l in program.derived for l, *_ in side[0]):
        return None
    return side


def bound_table(constraints: Sequence, trees: Trees, program, _slots=None) -> Bounds:
    """The table of ``mg_walk_bound``: the entries of
    :func:`aim_table` as XOR entries, in its order; then, for every MAGNITUDE
    atom of ``trees`` in atom order and after them for every simple MAGNITUDE
    root in root order (not one that is simple only because ``MAX_ATOMS`` was
    exceeded), an entry for side ``lo`` (LOW, LOW_STRICT for a strict order)
    and one for side ``hi`` (HIGH, HIGH_STRICT) where :func:`bound_side`
    resolves it.  At most 256 entries, the first ones."""
    constraints = list(constraints)
    aims = aim_table(trees, program, _slots)
    rows = [(int(p), aims.of(e), BOUND_XOR, 0, 0) for e, (p, _, _) in enumerate(aims.entries)]
    sides = list(aims.sides)

    def order(node, truth, negated=False):
        got = order_sides(node, negated)
        if got is None:
            return
        lo, hi, strict = got
        p = _order_probe(trees, lo, hi)
        if p is None:
            return
        for side, t in enumerate((lo, hi)):
            res = bound_side(t, program, _slots)
            if res is not None:
                rows.append((p, res[0], (BOUND_LOW, BOUND_HIGH)[side] + int(strict), truth, res[1]))
                sides.append(side)

    for i, e in enumerate(trees.atoms):
        if int(e) >> 16 == MAGNITUDE:
            order(trees.atom_nodes[i], BOUND_ATOM | i)
    for k, c in enumerate(constraints):
        if trees.is_tree(k) or trees.kind(k) != MAGNITUDE:
            continue
        d, neg = peel(c)
        if d.op not in _NEGATED_ORDER:                   # the classify fallback of a tree
            continue
        order(d, k, neg)
    out = make_bounds(rows[:AIM_MAX_ENTRIES], len(constraints), trees.n_atoms)
    out.sides = sides[:AIM_MAX_ENTRIES]
    return out


def bound_live_ref(state, bounds: Bounds) -> list:
    """L: the live entries in table order under ``state`` = (residual values
    (n_resid, 8) u32, root bits, atom bits) of the walker's base; empty for
    None (round 0).  An XOR entry is live iff its residual is not zero, an
    order entry iff its truth bit is clear."""
    if state is None:
        return []
    rv = np.asarray(state[0], dtype=np.uint32).reshape(-1, 8)
    live = []
    for e in range(len(bounds)):
        p, _, _, mode, truth = (int(x) for x in bounds.entries[e])
        if mode == BOUND_XOR:
            on = bool(rv[p].any())
        elif truth & BOUND_ATOM:
            on = not state[2][truth & ~BOUND_ATOM]
        else:
            on = not state[1][truth]
        if on:
            live.append(e)
    return live


def bound_picks_ref(state, bounds: Bounds, r: int, lanes: int) -> np.ndarray:
    """(lanes,) int64: the entry lane j of round ``r`` applies, or ``AIM_NONE``:
    :func:`aim_picks_ref`'s layout over the live list of :func:`bound_live_ref`."""
    out = np.full(lanes, AIM_NONE, dtype=np.int64)
    live = bound_live_ref(state, bounds)
    n1 = min(len(live), lanes // 8)
    for j in range(1, 2 * n1 + 1):
        out[j] = live[((j if j <= n1 else j - n1) - 1 + r * n1) % len(live)]
    return out


def bound_mutate_ref(leafgen, consts, base, state, bounds: Bounds, seed: int, r: int,
                     lanes: int) -> np.ndarray:
    """``[n_leaves][8][lanes]`` u32: the neighbours of ``base`` that round
    ``r`` of ``mg_walk_bound`` evaluates — the specification of
    ``csrc/mg_walk_bound.h``.  :func:`aim_mutate_ref` with the picks of
    :func:`bound_picks_ref`; an XOR entry acts as there, an order entry with
    residual value D and s = 1 if strict else 0 gathers ``V = fixed | OR
    ((base[leaf] >> leaf_bit) & mask(len)) << value_bit`` from the base, takes
    ``T = V - D - s`` (LOW) or ``V + D + s`` (HIGH) mod 2^256 and, in piece
    order, replaces bits ``leaf_bit ..`` of the lane's current value of the
    leaf by ``(T >> value_bit) & mask(len)``."""
    base = np.ascontiguousarray(base, dtype=np.uint32).reshape(-1, 8)
    picks = bound_picks_ref(state, bounds, r, lanes)
    n1 = int((picks != AIM_NONE).sum()) // 2
    out = np.repeat(base[:, :, None], lanes, axis=2)
    moves = moves_ref(leafgen, consts, base, seed, r, lanes)
    bvals = _ints(base)
    rv = _ints(np.asarray(state[0], dtype=np.uint32).reshape(-1, 8)) if n1 else []
    for lane in range(lanes):
        cur = {}
        if picks[lane] != AIM_NONE:
            e = int(picks[lane])
            p, _, _, mode, _ = (int(x) for x in bounds.entries[e])
            R = rv[p]
            if mode == BOUND_XOR:
                for leaf, leaf_bit, value_bit, n in bounds.of(e):
                    cur[leaf] = cur.get(leaf, bvals[leaf]) ^ (
                        (R >> value_bit & ((1 << n) - 1)) << leaf_bit)
            else:
                V = bounds.fixed_of(e)
                for leaf, leaf_bit, value_bit, n in bounds.of(e):
                    V |= (bvals[leaf] >> leaf_bit & ((1 << n) - 1)) << value_bit
                s = 1 if mode in (BOUND_LOW_STRICT, BOUND_HIGH_STRICT) else 0
                T = (V - R - s if mode <= BOUND_LOW_STRICT else V + R + s) & M256
                for leaf, leaf_bit, value_bit, n in bounds.of(e):
                    m = (1 << n) - 1
                    cur[leaf] = (cur.get(leaf, bvals[leaf]) & ~(m << leaf_bit)) | (
                        (T >> value_bit & m) << leaf_bit)
        if lane > n1:
            for leaf, _, v in moves[lane]:
                cur[leaf] = v
        for leaf, v in cur.items():
            out[leaf, :, lane] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    return out


# ---------------------------------------------------------------------------
# aims for UF outputs: a piece may name a UF slot, whose
# destination leaf is resolved at every adoption
# ---------------------------------------------------------------------------

# the constants of csrc/mg_walk_uf.h
UF_SLOT = 1 << 31
UF_MAX_SLOTS, UF_MAX_FUNCS, UF_MAX_CANDS, UF_MAX_ROWS, UF_MAX_CHUNKS = 64, 64, 256, 128, 4
UF_CONST, UF_LEAF, UF_PROBE, UF_ALWAYS = range(4)


@dataclass
class Ufs:
    """The UF tables of ``mg_walk_uf`` (``csrc/mg_walk_uf.h``)."""
    slots: np.ndarray          # (n_slots, 2) u32: function, first U row of the argument
    funcs: np.ndarray          # (n_funcs, 3) u32: first candidate, candidates, key chunks
    cands: np.ndarray          # (n_cands, 6) u32: value leaf | AIM_NONE, key kind, key words
    ukeys: np.ndarray          # (n_ukeys, 8) u32: the chunks of the constant keys
    n_urows: int = 0           # argument rows, then kept key rows
    n_arg_rows: int = 0        # the argument probes the walk view keeps (the first ones)
    keep: tuple = ()           # probe indices of the kept entry keys (uf_view)
    apps: tuple = ()           # per slot its ``apply`` node
    names: tuple = ()          # per function its name
    slot_of: Optional[dict] = None      # apply node id -> slot
    underived: frozenset = frozenset()  # apply node ids refused because every value is derived

    def __len__(self) -> int:
        return len(self.slots)


def make_ufs(slots=(), funcs=(), cands=(), ukeys=(), n_urows: int = 0) -> Ufs:
    """``Ufs`` of plain rows (``ukeys``: ints or 8-limb rows)."""
    keys = [_u256(k) if isinstance(k, int) else k for k in ukeys]
    return Ufs(np.array(slots, dtype=np.uint32).reshape(-1, 2),
               np.array(funcs, dtype=np.uint32).reshape(-1, 3),
               np.array(cands, dtype=np.uint32).reshape(-1, 6),
               np.array(keys, dtype=np.uint32).reshape(-1, 8), n_urows, n_urows)


def no_ufs() -> Ufs:
    return make_ufs()


def _read_probes(trees: Trees) -> list:
    """The residual probes a HAMMING or MAGNITUDE atom or simple root of
    ``trees`` reads, in probe order."""
    used = set()
    for e in list(trees.atoms) + [r for r in trees.roots if not int(r) & WT_TREE]:
        if int(e) >> 16 in (HAMMING, MAGNITUDE):
            used.add(int(e) & 0xFFFF)
    return sorted(used)


def _arg_chunks(t) -> list:
    """The argument of the application ``t`` as 256-bit chunks, low first."""
    a = t.args[0]
    return [_chunk(a, min(lo + RESIDUAL_BITS, a.width) - 1, lo)
            for lo in range(0, a.width, RESIDUAL_BITS)]


def uf_probes(trees: Trees) -> tuple:
    """``(apps, probes)`` from the nodes alone: the ``apply``
    nodes met on either side of every residual probe ``bvxor(a, b)`` /
    ``bvsub(lo, hi)`` that a HAMMING or MAGNITUDE atom or simple root of
    ``trees`` reads, by the destination rules of :func:`aim_pieces` (through
    ``concat``, ``extract``, ``zero_extend`` and an ``ite`` with a numeral
    arm), distinct by id in first-seen order; kept where the range is at most
    256 bits, the domain at most 1024 (4 chunks) and the argument no numeral;
    at most 64, the first ones.  ``probes``: their arguments cut into 256-bit
    chunks, low chunk first, to compile as user probes after the residuals."""
    apps, seen = [], set()

    def go(t):
        if t.op == "apply":
            if t.id not in seen:
                seen.add(t.id)
                apps.append(t)
        elif t.op == "concat":
            for a in t.args:
                go(a)
        elif t.op in ("extract", "zero_extend"):
            go(t.args[0])
        elif t.op == "ite" and t.is_bv():
            _, x, y = t.args
            if x.op == "bvnum" or y.op == "bvnum":
                go(y if x.op == "bvnum" else x)

    for p in _read_probes(trees):
        node = trees.probes[p]
        if node.op in ("bvxor", "bvsub") and len(node.args) == 2:
            for t in node.args:
                go(t)
    apps = [t for t in apps if t.width <= RESIDUAL_BITS
            and t.params[1] <= RESIDUAL_BITS * UF_MAX_CHUNKS and t.args[0].op != "bvnum"]
    apps = apps[:UF_MAX_SLOTS]
    return apps, [c for t in apps for c in _arg_chunks(t)]


def uf_view(program, n_user: int, keep: Sequence[int]):
    """``census.census_view`` extended: ``program`` with its first ``n_user``
    probes kept, the ``OUT`` records of the probe indices in ``keep``
    renumbered to ``n_user``, ``n_user + 1``, .. and every other ``OUT``
    replaced by ``NOP``."""
    import copy
    from . import irdefs as I
    keep = [int(k) for k in keep]
    if not 1 <= n_user <= program.n_probes or any(not n_user <= k < program.n_probes for k in keep) \
            or len(set(keep)) != len(keep):
        raise ValueError("n_user %d or a kept probe outside the program's %d probes" % (
            n_user, program.n_probes))
    code = np.array(program.code, dtype=np.uint32, copy=True)
    out = (code[:, 0] & 0xFF) == I.OUT
    where = {k: n_user + i for i, k in enumerate(keep)}
    for i in np.flatnonzero(out & (code[:, 2] >= n_user)):
        k = int(code[i, 2])
        if k in where:
            code[i, 2] = where[k]
        else:
            code[i] = (I.NOP, 0, 0, 0)
    view = copy.copy(program)
    view.code = code
    view.n_probes = n_user + len(keep)
    return view


def uf_table(constraints: Sequence, trees: Trees, program, apps: Sequence) -> tuple:
    """``(Bounds, Ufs)`` of ``mg_walk_uf`` on ``program``,
    compiled with the argument probes of ``apps`` (:func:`uf_probes`) as its
    last user probes.  Per function the candidates stand in the table's
    precedence order: the ``table_ckeys`` entries (CONST keys, value leaf kind
    ``cval``), then the leaf-keyed (eval form: LEAF keys) or argument-keyed
    (solve form: PROBE keys, ``Program.entry_keys``) entries (value leaf kind
    ``val``), then in eval form ``else`` (ALWAYS).  A candidate whose value
    leaf the program derives keeps its place with value leaf ``AIM_NONE``.
    An application all of whose candidates are so gets no slot; the later
    slots are dropped, and with them the key rows of a function no slot is
    left of, until there are at most 64 slots, 256 candidates and 128 U rows.
    The ``Bounds`` are :func:`bound_table`'s with slot pieces."""
    apps = list(apps)
    leaves = {(l.kind, l.source, l.entry, l.chunk): i for i, l in enumerate(program.leaves)}

    def candidates(t):
        """[(value leaf, kind, keys)] of t's function; keys: ints (CONST),
        leaves (LEAF) or probe indices (PROBE)."""
        name, chunks = t.params[0], (t.params[1] + RESIDUAL_BITS - 1) // RESIDUAL_BITS

        def value(kind, e):
            li = leaves.get((kind, name, e, 0))
            return AIM_NONE if li is None or li in program.derived or \
                program.leaves[li].width != t.width else li
        out = [(value("cval", i), UF_CONST,
                [key >> (RESIDUAL_BITS * k) & M256 for k in range(chunks)])
               for i, key in enumerate(program.table_ckeys.get(name, []))]
        if name in program.entry_keys:
            out += [(value("val", e), UF_PROBE, list(key))
                    for e, key in enumerate(program.entry_keys[name])]
        else:
            for e in range(program.table_sizes.get(name, 0)):
                keys = [leaves.get(("key", name, e, k)) for k in range(chunks)]
                if None not in keys:
                    out.append((value("val", e), UF_LEAF, keys))
            out.append((value("else", 0), UF_ALWAYS, []))
        return out

    cands_of = {}
    for t in apps:
        if t.params[0] not in cands_of:
            cands_of[t.params[0]] = candidates(t)
    underived = frozenset(t.id for t in apps
                          if all(v == AIM_NONE for v, _, _ in cands_of[t.params[0]]))
    arg_row, row = {}, 0
    for t in apps:
        arg_row[t.id] = row
        row += len(_arg_chunks(t))
    kept = [t for t in apps if t.id not in underived][:UF_MAX_SLOTS]
    while kept:
        names = list(dict.fromkeys(t.params[0] for t in kept))
        n_arg = arg_row[kept[-1].id] + len(_arg_chunks(kept[-1]))
        n_key = sum(len(key) for n in names for _, kind, key in cands_of[n] if kind == UF_PROBE)
        if len(names) <= UF_MAX_FUNCS and n_arg + n_key <= UF_MAX_ROWS and \
                sum(len(cands_of[n]) for n in names) <= UF_MAX_CANDS:
            break
        kept.pop()
    if not kept:                                         # (the reasons stay: aim_refusal)
        none = no_ufs()
        none.slot_of, none.underived = {}, underived
        return bound_table(constraints, trees, program), none
    keep, ukeys, funcs, cands, findex = [], [], [], [], {}
    for n in names:
        findex[n] = len(funcs)
        chunks = (next(t for t in kept if t.params[0] == n).params[1] + RESIDUAL_BITS - 1) \
            // RESIDUAL_BITS
        funcs.append((len(cands), len(cands_of[n]), chunks))
        for v, kind, key in cands_of[n]:
            words = []
            for k in key:
                if kind == UF_CONST:
                    words.append(len(ukeys))
                    ukeys.append(_u256(k))
                elif kind == UF_PROBE:
                    words.append(n_arg + len(keep))
                    keep.append(int(k))
                else:
                    words.append(k)
            cands.append([v, kind] + words + [0] * (UF_MAX_CHUNKS - len(words)))
    slot_of = {t.id: u for u, t in enumerate(kept)}
    ufs = Ufs(np.array([(findex[t.params[0]], arg_row[t.id]) for t in kept],
                       dtype=np.uint32).reshape(-1, 2),
              np.array(funcs, dtype=np.uint32).reshape(-1, 3),
              np.array(cands, dtype=np.uint32).reshape(-1, 6),
              np.array(ukeys, dtype=np.uint32).reshape(-1, 8), n_arg + len(keep), n_arg,
              tuple(keep), tuple(kept), tuple(names), slot_of, underived)
    return bound_table(constraints, trees, program, _slots=slot_of), ufs


def has_slot_piece(bounds: Bounds) -> bool:
    return bool(len(bounds.pieces)) and bool((bounds.pieces[:, 0] & UF_SLOT).any())


def uf_resolve_ref(base, urows, ufs: Ufs) -> np.ndarray:
    """(n_slots,) u32: the destination leaf of every slot under ``base``
    ((n_leaves, 8) u32, the adopted lane already applied) and the adopted
    lane's U rows ``urows`` ((n_urows, 8) u32) — the specification of
    ``mg_walk_uf_resolve``.  The destination is the value leaf of the FIRST
    candidate of the slot's function whose key equals the argument's rows in
    every chunk and limb (ALWAYS matches); ``AIM_NONE`` when none matches or
    that candidate has no value leaf."""
    base = np.asarray(base, dtype=np.uint32).reshape(-1, 8)
    urows = np.asarray(urows, dtype=np.uint32).reshape(-1, 8)
    out = np.full(len(ufs.slots), AIM_NONE, dtype=np.uint32)
    for u, (f, arg) in enumerate(ufs.slots.tolist()):
        first, cnt, chunks = (int(x) for x in ufs.funcs[f])
        for c in range(first, first + cnt):
            v, kind = int(ufs.cands[c, 0]), int(ufs.cands[c, 1])
            hit = True
            for k in range(chunks if kind != UF_ALWAYS else 0):
                key = int(ufs.cands[c, 2 + k])
                row = (ufs.ukeys[key] if kind == UF_CONST else base[key] if kind == UF_LEAF
                       else urows[key])
                hit = hit and bool((row == urows[arg + k]).all())
            if hit:
                out[u] = v
                break
    return out


def _uf_leaf(leaf: int, dest) -> int:
    return int(dest[leaf & ~UF_SLOT]) if leaf & UF_SLOT else leaf


def uf_live_ref(state, bounds: Bounds) -> list:
    """L under ``state`` = (residual values, root bits, atom bits, slot
    destinations (n_slots,)): :func:`bound_live_ref`'s, without the entries
    that have a slot piece whose destination is ``AIM_NONE``."""
    if state is None:
        return []
    return [e for e in bound_live_ref(state[:3], bounds)
            if all(_uf_leaf(leaf, state[3]) != AIM_NONE for leaf, *_ in bounds.of(e))]


def uf_picks_ref(state, bounds: Bounds, r: int, lanes: int) -> np.ndarray:
    """:func:`bound_picks_ref` over the live list of :func:`uf_live_ref`."""
    out = np.full(lanes, AIM_NONE, dtype=np.int64)
    live = uf_live_ref(state, bounds)
    n1 = min(len(live), lanes // 8)
    for j in range(1, 2 * n1 + 1):
        out[j] = live[((j if j <= n1 else j - n1) - 1 + r * n1) % len(live)]
    return out


def uf_mutate_ref(leafgen, consts, base, state, bounds: Bounds, seed: int, r: int,
                  lanes: int) -> np.ndarray:
    """``[n_leaves][8][lanes]`` u32: the neighbours of ``base`` that round
    ``r`` of ``mg_walk_uf`` evaluates — the specification of
    ``csrc/mg_walk_uf.h``.  :func:`bound_mutate_ref` with the picks of
    :func:`uf_picks_ref`, where a slot piece ``UF_SLOT | u`` acts on the leaf
    ``state[3][u]`` wherever a piece acts on its leaf: the gather of V, the
    scatter, and the plain move that wins a leaf it shares with a piece."""
    base = np.ascontiguousarray(base, dtype=np.uint32).reshape(-1, 8)
    picks = uf_picks_ref(state, bounds, r, lanes)
    n1 = int((picks != AIM_NONE).sum()) // 2
    out = np.repeat(base[:, :, None], lanes, axis=2)
    moves = moves_ref(leafgen, consts, base, seed, r, lanes)
    bvals = _ints(base)
    rv = _ints(np.asarray(state[0], dtype=np.uint32).reshape(-1, 8)) if n1 else []
    for lane in range(lanes):
        cur = {}
        if picks[lane] != AIM_NONE:
            e = int(picks[lane])
            p, _, _, mode, _ = (int(x) for x in bounds.entries[e])
            R = rv[p]
            ps = [(_uf_leaf(leaf, state[3]), lb, vb, n) for leaf, lb, vb, n in bounds.of(e)]
            if mode == BOUND_XOR:
                for leaf, leaf_bit, value_bit, n in ps:
                    cur[leaf] = cur.get(leaf, bvals[leaf]) ^ (
                        (R >> value_bit & ((1 << n) - 1)) << leaf_bit)
            else:
                V = bounds.fixed_of(e)
                for leaf, leaf_bit, value_bit, n in ps:
                    V |= (bvals[leaf] >> leaf_bit & ((1 << n) - 1)) << value_bit
                s = 1 if mode in (BOUND_LOW_STRICT, BOUND_HIGH_STRICT) else 0
                T = (V - R - s if mode <= BOUND_LOW_STRICT else V + R + s) & M256
                for leaf, leaf_bit, value_bit, n in ps:
                    m = (1 << n) - 1
                    cur[leaf] = (cur.get(leaf, bvals[leaf]) & ~(m << leaf_bit)) | (
                        (T >> value_bit & m) << leaf_bit)
        if lane > n1:
            for leaf, _, v in moves[lane]:
                cur[leaf] = v
        for leaf, v in cur.items():
            out[leaf, :, lane] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    return out


# ---------------------------------------------------------------------------
# aims through sums: a side that is a sum of +-terms moves
# by moving one of its terms
# ---------------------------------------------------------------------------

# the constants of csrc/mg_walk_sum.h
SUM_LINEAR, SUM_NEG, SUM_ROW_SHIFT = 1, 2, 8
SUM_MAX_ROWS, SUM_MAX_TERMS = 64, 4


@dataclass
class Sums:
    """What ``mg_walk_sum`` adds to the tables of ``mg_walk_uf``
    (``csrc/mg_walk_sum.h``)."""
    lin: np.ndarray            # (n_entries,) u32: 0, or LINEAR | NEG? | side row << 8
    n_srows: int = 0           # side rows the program writes after the residuals
    probes: tuple = ()         # per side row its node (sum_probes)

    @property
    def n_linear(self) -> int:
        return int((self.lin != 0).sum())


def no_sums(n_entries: int = 0) -> Sums:
    return Sums(np.zeros(n_entries, dtype=np.uint32))


def make_sums(words, n_srows: int = 0) -> Sums:
    """``Sums`` of one ``None`` (not linear) or ``(sign, side row)`` per entry."""
    lin = [0 if w is None else SUM_LINEAR | (SUM_NEG if w[0] < 0 else 0) | w[1] << SUM_ROW_SHIFT
           for w in words]
    return Sums(np.array(lin, dtype=np.uint32).reshape(-1), n_srows)


def linear_terms(t) -> Optional[list]:
    """``[(sign, term)]``, the non-numeral terms of the side ``t`` in order,
    when ``t`` is linear by its nodes: at most 256 bits
    wide, a ``bvadd``, ``bvsub`` or ``bvneg`` at the top, and 1 .. 4 terms
    after flattening ``bvadd`` (n-ary, nested), ``bvsub(x, y)`` as ``x + (-y)``
    and ``bvneg``; numerals are dropped (the move is a difference).  Else
    None.  Nothing under another operator is flattened."""
    if not t.is_bv() or t.width > RESIDUAL_BITS or t.op not in ("bvadd", "bvsub", "bvneg"):
        return None
    out = []

    def go(t, sign):
        if t.op == "bvadd":
            for a in t.args:
                go(a, sign)
        elif t.op == "bvsub":
            go(t.args[0], sign)
            go(t.args[1], -sign)
        elif t.op == "bvneg":
            go(t.args[0], -sign)
        elif t.op != "bvnum":
            out.append((sign, t))
    go(t, 1)
    return out if 1 <= len(out) <= SUM_MAX_TERMS else None


def _names(t) -> set:
    """The names of the variables, arrays and functions under ``t``."""
    out, seen, todo = set(), set(), [t]
    while todo:
        n = todo.pop()
        if n.id in seen:
            continue
        seen.add(n.id)
        if n.op in ("var", "array", "apply"):
            out.add(n.params[0])
        todo.extend(n.args)
    return out


def sum_target(t, i: int, program, slots=None):
    """Term ``i`` of the linear side ``t`` as a target: ``(sign, pieces,
    fixed)`` when it is eligible, else the reason as a string.  Eligible: it
    resolves with the rules of §3.15 to 1 .. 64 pieces, none a UF slot, none
    on a leaf the program derives, and no variable, array or function its
    leaves come from occurs under another term of the side."""
    terms = linear_terms(t)
    sign, x = terms[i]
    res = _resolve_side(x, program, slots, True)
    if res is None:
        return aim_refusal(x, program, None, True) or "%s is not a destination" % x.op
    ps, fixed = res
    if not ps:
        return "a term without a piece"
    if len(ps) > AIM_MAX_PIECES:
        return "a term of more than %d pieces" % AIM_MAX_PIECES
    if any(l & UF_SLOT for l, *_ in ps):
        return "a UF slot piece in a sum"
    if any(l in program.derived for l, *_ in ps):
        return "a term on a derived leaf"
    mine = {program.leaves[l].source for l, *_ in ps}
    for k, (_, other) in enumerate(terms):
        if k != i and mine & _names(other):
            return "a leaf shared with another term"
    return sign, ps, fixed


def sum_probes(trees: Trees) -> list:
    """The linear sides that need a side row, from the nodes alone (DESIGN.md
    §3.15): the sides of every residual probe ``bvxor(a, b)`` that a HAMMING
    atom or simple root of ``trees`` reads, in probe order, ``a`` then ``b``,
    that :func:`linear_terms` takes; distinct by id in first-seen order; at
    most 64, the first ones.  Compiled as user probes after the residuals."""
    out, seen = [], set()
    for p in _read_probes(trees):
        node = trees.probes[p]
        if node.op != "bvxor" or len(node.args) != 2:
            continue
        e = [int(x) for x in list(trees.atoms) + [r for r in trees.roots if not int(r) & WT_TREE]
             if int(x) & 0xFFFF == p]
        if not any(x >> 16 == HAMMING for x in e):
            continue
        for t in node.args:
            if t.id not in seen and linear_terms(t) is not None:
                seen.add(t.id)
                out.append(t)
    return out[:SUM_MAX_ROWS]


def sum_table(constraints: Sequence, trees: Trees, program, apps: Sequence) -> tuple:
    """``(Bounds, Ufs, Sums)`` of ``mg_walk_sum`` on
    ``program``, compiled with the side rows of :func:`sum_probes` after the
    residuals and the argument probes of ``apps`` after them.  The ``Ufs`` are
    :func:`uf_table`'s.  The entries follow its procedure and order — the XOR
    entries of :func:`aim_table`, then the order entries of
    :func:`bound_table` — with the mask and shift rules of §3.15 on: where a
    side resolves it gives the entry it gives there (``lin`` 0); else, where
    :func:`linear_terms` takes it, one entry per eligible target
    (:func:`sum_target`) in term order, with the side's row, mode and truth
    and the target's pieces and fixed bits, ``lin`` = LINEAR, NEG for a
    negative term and, in XOR mode, the side's row among :func:`sum_probes`
    (a side past the 64 rows gets no XOR entry).  At most 256 entries, the
    first ones."""
    constraints = list(constraints)
    _, ufs = uf_table(constraints, trees, program, apps)
    slots = ufs.slot_of if len(ufs) else None
    sides_with_row = sum_probes(trees)
    row_of = {t.id: i for i, t in enumerate(sides_with_row)}
    rows, sides, words = [], [], []

    def side_entries(p, t, side, mode, truth):
        res = _resolve_side(t, program, slots, True)
        if res is not None:
            if res[0] and len(res[0]) <= AIM_MAX_PIECES and \
                    not any(l in program.derived for l, *_ in res[0]):
                rows.append((p, res[0], mode, truth, 0 if mode == BOUND_XOR else res[1]))
                sides.append(side)
                words.append(None)
            return
        terms = linear_terms(t)
        if terms is None or (mode == BOUND_XOR and t.id not in row_of):
            return
        for i in range(len(terms)):
            got = sum_target(t, i, program, slots)
            if isinstance(got, str):
                continue
            sign, ps, fixed = got
            rows.append((p, ps, mode, truth, fixed))
            sides.append(side)
            words.append((sign, row_of[t.id] if mode == BOUND_XOR else 0))

    used = set()
    for e in list(trees.atoms) + [r for r in trees.roots if not int(r) & WT_TREE]:
        if int(e) >> 16 == HAMMING:
            used.add(int(e) & 0xFFFF)
    for p in sorted(used):
        node = trees.probes[p]
        if node.op != "bvxor" or len(node.args) != 2:
            continue
        for side, t in enumerate(node.args):
            side_entries(p, t, side, BOUND_XOR, 0)

    def order(node, truth, negated=False):
        got = order_sides(node, negated)
        if got is None:
            return
        lo, hi, strict = got
        p = _order_probe(trees, lo, hi)
        if p is None:
            return
        for side, t in enumerate((lo, hi)):
            side_entries(p, t, side, (BOUND_LOW, BOUND_HIGH)[side] + int(strict), truth)

    for i, e in enumerate(trees.atoms):
        if int(e) >> 16 == MAGNITUDE:
            order(trees.atom_nodes[i], BOUND_ATOM | i)
    for k, c in enumerate(constraints):
        if trees.is_tree(k) or trees.kind(k) != MAGNITUDE:
            continue
        d, neg = peel(c)
        if d.op not in _NEGATED_ORDER:
            continue
        order(d, k, neg)
    bounds = make_bounds(rows[:AIM_MAX_ENTRIES], len(constraints), trees.n_atoms)
    bounds.sides = sides[:AIM_MAX_ENTRIES]
    sums = make_sums(words[:AIM_MAX_ENTRIES], len(sides_with_row))
    sums.probes = tuple(sides_with_row)
    return bounds, ufs, sums


def sum_mutate_ref(leafgen, consts, base, state, bounds: Bounds, sums: Sums, seed: int, r: int,
                   lanes: int) -> np.ndarray:
    """``[n_leaves][8][lanes]`` u32: the neighbours of ``base`` that round
    ``r`` of ``mg_walk_sum`` evaluates — the specification of
    ``csrc/mg_walk_sum.h``.  :func:`uf_mutate_ref` (its picks and live list
    too) under ``state`` = (residual values, root bits, atom bits, slot
    destinations, side rows (n_srows, 8) u32), where a linear entry (``sums.lin``)
    gathers its target's value ``V = fixed | OR ((base[leaf] >> leaf_bit) &
    mask(len)) << value_bit``, takes with R its residual value, s = 1 for the
    strict modes and S its side row's value
    ``X = V - sign (R + s)`` (LOW), ``V + sign (R + s)`` (HIGH) or ``V + sign
    ((S ^ R) - S)`` (XOR) mod 2^256, and replaces, in piece order, bits
    ``leaf_bit ..`` of the lane's current value of the leaf by ``(X >>
    value_bit) & mask(len)``."""
    base = np.ascontiguousarray(base, dtype=np.uint32).reshape(-1, 8)
    picks = uf_picks_ref(state, bounds, r, lanes)
    n1 = int((picks != AIM_NONE).sum()) // 2
    out = np.repeat(base[:, :, None], lanes, axis=2)
    moves = moves_ref(leafgen, consts, base, seed, r, lanes)
    bvals = _ints(base)
    rv = _ints(np.asarray(state[0], dtype=np.uint32).reshape(-1, 8)) if n1 else []
    sv = _ints(np.asarray(state[4], dtype=np.uint32).reshape(-1, 8)) if n1 else []
    for lane in range(lanes):
        cur = {}
        if picks[lane] != AIM_NONE:
            e = int(picks[lane])
            p, _, _, mode, _ = (int(x) for x in bounds.entries[e])
            R, lw = rv[p], int(sums.lin[e])
            ps = [(_uf_leaf(leaf, state[3]), lb, vb, n) for leaf, lb, vb, n in bounds.of(e)]
            if mode == BOUND_XOR and not lw:
                for leaf, leaf_bit, value_bit, n in ps:
                    cur[leaf] = cur.get(leaf, bvals[leaf]) ^ (
                        (R >> value_bit & ((1 << n) - 1)) << leaf_bit)
            else:
                V = bounds.fixed_of(e)
                for leaf, leaf_bit, value_bit, n in ps:
                    V |= (bvals[leaf] >> leaf_bit & ((1 << n) - 1)) << value_bit
                s = 1 if mode in (BOUND_LOW_STRICT, BOUND_HIGH_STRICT) else 0
                up = mode >= BOUND_HIGH
                d = R + s
                if lw:
                    if mode == BOUND_XOR:
                        S = sv[lw >> SUM_ROW_SHIFT & 0xFF]
                        d, up = (S ^ R) - S, True
                    if lw & SUM_NEG:
                        up = not up
                T = (V + d if up else V - d) & M256
                for leaf, leaf_bit, value_bit, n in ps:
                    m = (1 << n) - 1
                    cur[leaf] = (cur.get(leaf, bvals[leaf]) & ~(m << leaf_bit)) | (
                        (T >> value_bit & m) << leaf_bit)
        if lane > n1:
            for leaf, _, v in moves[lane]:
                cur[leaf] = v
        for leaf, v in cur.items():
            out[leaf, :, lane] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    return out


# ---------------------------------------------------------------------------
# repair a missed group
# ---------------------------------------------------------------------------

REPAIRED, STUCK = "repaired", "stuck"


def repair_group(nodes: Sequence, n_cand: int = 1 << 16, form: str = "search", lanes: int = 4096,
                 max_rounds: int = 64, device: int = 0, seed: Optional[int] = None,
                 sync_every: int = 8, scored=False, walkers: int = 1) -> dict:
    """Census, then local search, of ONE independent group (root k =
    ``nodes[k]``): the statuses of ``census.explain_group`` for a group that
    launches nothing, else ``repaired`` with ``assignment`` (a model of the
    group) or ``stuck``; a launched group also reports ``census``, ``start``
    (index and failing constraints of the census's best candidate) and
    ``repair`` (the :class:`RepairResult`; None when the census itself found
    a satisfying candidate).  The search runs on the census view from the
    leaves of ``best_index``; the verdict is a fresh evaluation of the full
    masked program on the returned leaves — root bit and every mask bit set
    — not the loop's counter.  In solve form only the free leaves move: the
    construction's definitions recompute the rest.

    ``scored``: the scored walk (``mg_walk``) of ``walkers``
    walkers instead: the program also carries the residual probes of
    :func:`residuals`, ``repair`` is a :class:`WalkResult` and ``starts`` the
    candidate indices the walkers left from — the census's ``best_index``,
    then ``sole_index`` of its ``blockers()`` in rank order without
    duplicates, then ``best_index`` again; ``table`` is the residual table
    and, when the walk is stuck, ``failing`` the roots its winner still
    fails.  The verdict is the same fresh evaluation, of the winner's
    leaves.

    ``scored="tree"``: the same walk scored by distance trees
    (``mg_walk_tree``): the program carries the root mask,
    the atom mask and the residual probes of :func:`distance_trees`
    (``trees`` in the result), same starts, same acceptance.  When that
    program does not compile, or the compiler folds a probe away, the group
    falls back to the table of ``scored=True`` and then to the count;
    ``scoring`` says which ran: ``"tree"``, ``"table"`` or ``"count"``.  A
    stuck tree walk also reports ``atom_state``: per atom whether it holds on
    the winner and, if not, its distance.

    ``scored="aim"``: the tree-scored walk with aimed moves (``mg_walk_aim``,
    DESIGN.md §3.12): compiled as ``"tree"``, then the aim table of
    :func:`aim_table` on the compiled program (``aims`` in the result); with
    no entry, and where ``"tree"`` falls back, it runs as ``"tree"`` does;
    ``scoring`` is ``"aim"`` when aimed moves ran, and ``program`` is the
    compiled program whose leaves the table names.

    ``scored="bound"``: the same with aims for orders too (``mg_walk_bound``,
    DESIGN.md §3.13): compiled as ``"tree"``, then the table of
    :func:`bound_table` on the compiled program (``bounds`` in the result);
    ``scoring`` is ``"bound"`` when the table has an order entry, else the
    group runs exactly as ``scored="aim"`` does.

    ``scored="uf"``: the same with aims that write the table entry a UF
    application reads (``mg_walk_uf``): compiled as
    ``"tree"`` plus the argument probes of :func:`uf_probes`, then the tables
    of :func:`uf_table` (``bounds`` and ``ufs`` in the result); ``scoring`` is
    ``"uf"`` when a slot piece is in the table.  When that program does not
    compile, a probe is folded away or no slot piece results, the group runs
    exactly as ``scored="bound"`` does.

    ``scored="sum"``: the same with aims through sums, differences, masks and
    shifts (``mg_walk_sum``): compiled as ``"uf"`` plus the
    side rows of :func:`sum_probes` between the residuals and the argument
    probes, then the tables of :func:`sum_table` (``bounds``, ``ufs`` and
    ``sums`` in the result); ``scoring`` is ``"sum"`` when a linear entry is in
    the table.  When that program does not compile or a probe is folded away,
    the group falls back to ``"uf"`` and onward; with no linear entry it runs
    exactly as ``scored="uf"`` does on the table of :func:`sum_table` (the
    mask and shift rules may have added plain entries to it)."""
    steps = _repair_steps(nodes, n_cand, form, lanes, max_rounds, device, seed, sync_every, scored,
                          walkers)
    try:
        step = next(steps)
        while True:
            step = steps.send(step.single())
    except StopIteration as done:
        return done.value


class _CensusJob:
    """Where :func:`_repair_steps` hands the census of its group to its driver:
    ``single()`` is the ``Engine.census`` call :func:`repair_group` always
    made; ``job`` is the same census as a job of ``Engine.census_batch`` on
    ``eng`` (every group of a call shares seed, range and chunk)."""
    stage = 0

    def __init__(self, eng, view, n_roots, n_cand):
        self.eng, self.view, self.n_roots, self.n_cand = eng, view, n_roots, n_cand
        self.job = (view, n_roots, 0)

    def single(self):
        from . import model as M
        return self.eng.census(self.view, M.SEARCH_SEED, 0, self.n_cand, self.n_roots, 0)


class _CarryCensusJob:
    """Where :func:`_repair_steps` with ``carried`` hands the census of its
    ladder to its driver: ``job`` is a job of ``Engine.carry_census`` on
    ``eng``; the answer is that call's ``(censuses, start_col, start_nfail,
    starts)`` for it.  ``free``: some rung has a free leaf (else one lane says
    all).  ``single()`` is the call for this job alone at ``carry.CARRY_LANES``;
    :func:`repair_carried` serves all groups of an engine with one call."""
    stage = 0

    def __init__(self, eng, view, rows, masks, n_roots, walkers, free):
        self.eng, self.walkers, self.free = eng, walkers, free
        self.job = (view, rows, masks, n_roots)

    def single(self, lanes=None):
        from . import carry as CY
        from . import model as M
        lanes = CY.CARRY_LANES if lanes is None else lanes
        return self.eng.carry_census([self.job], M.SEARCH_SEED, 0, lanes if self.free else 1,
                                     self.walkers)[0]


class _WitnessJob:
    """Where :func:`_repair_steps` asks for the leaves of the candidates
    ``picks`` of the full masked program: a list of (n_leaves, 8) rows, one per
    pick.  ``single()`` makes the ``Engine.witness`` calls :func:`repair_group`
    always made, one per distinct index in the order of ``picks``; ``pairs``
    are the same as pairs of ``Engine.batch_witness`` on ``eng``."""
    stage = 1

    def __init__(self, eng, full, picks):
        self.eng, self.full, self.picks = eng, full, list(picks)
        self.pairs = [(full, i) for i in self.picks]

    def single(self):
        from . import model as M
        rows = {}
        for i in self.picks:
            if i not in rows:
                rows[i] = self.eng.witness(self.full, M.SEARCH_SEED, i)[0]
        return [rows[i] for i in self.picks]


class _TreeWalk:
    """Where :func:`_repair_steps` hands a tree-scored walk to its driver:
    ``job`` is the walk as a job of ``Engine.walk_batch`` on ``eng``
    (mg_walk_sum's arguments: a kind without a table gets the empty one, which
    by §3.12 - §3.15 is that kind bit for bit); ``single()`` runs it as
    :func:`repair_group` always has, with the entry of its own ``rung``
    (``Engine.walk_<rung>``) on the tables of the job that the entry takes."""

    stage = 2

    def __init__(self, eng, rung, job, lanes, max_rounds, sync_every):
        self.eng, self.rung, self.job = eng, rung, job
        self.how = (lanes, max_rounds, sync_every)

    def single(self):
        wide, starts, n, trees, bounds, ufs, sums, seed = self.job
        tables = {"tree": (), "bound": (bounds,), "uf": (bounds, ufs), "sum": (bounds, ufs, sums),
                  # the job's XOR entries are the aim table's with two zero words each
                  "aim": (Aims(bounds.entries[:, :3], bounds.pieces, bounds.sides),)}[self.rung]
        return getattr(self.eng, "walk_" + self.rung)(wide, starts, n, trees, *tables, seed,
                                                      *self.how)


def _repair_steps(nodes, n_cand, form, lanes, max_rounds, device, seed, sync_every, scored,
                  walkers, carried=None):
    """:func:`repair_group` in three steps, as a generator.  Prepare: compile,
    build the tables, then two hand-overs: the census is yielded as a
    :class:`_CensusJob` and its ``Census`` sent back, and the starts, picked
    from it here on the host, as a :class:`_WitnessJob` whose rows are sent
    back.  Walk: a tree-scored walk is yielded as a :class:`_TreeWalk` and its
    ``WalkResult`` sent back.  :func:`repair_group` serves every hand-over with
    the single call, :func:`repair_groups` with one batched call for all
    groups; the table-scored walk and the count walk run here.  Finish: the
    fresh evaluation, ``failing``, ``atom_state``, the assignment.  Returns the
    group's dict.

    ``carried``: an ``(assignment, taken_keys)`` pair of ``carry.plan`` — the
    walk from the carried starts of DESIGN.md §3.20.  The programs are the
    constant-keyed eval form of the carry (``carry.compile_census_ck``, the
    table sizes of ``carry.table_sizes_ck``) with the same probe lists and
    fallbacks, loaded with ``model.search_leafgen``; the census hand-over is a
    :class:`_CarryCensusJob` (stage 0) whose answer — the censuses of the
    ladder's rungs, the start columns, their failing roots and their rows —
    replaces both the census and the witness hand-over: ``census`` is the
    per-rung list, ``rungs`` the kept rung indices, ``start`` ``{"col", "rung",
    "nfail"}`` of start 0 and ``starts`` the columns.  A start 0 that fails no
    root goes straight to the fresh evaluation; else the walk runs as ever."""
    from . import census as CS
    from . import model as M
    from .assign import unpack
    from .engine import get_engine
    from .ir import Unsupported
    from .refute import refuted
    if form not in ("search", "eval"):
        raise ValueError("form must be 'search' or 'eval'")
    nodes = list(nodes)
    out: dict = {"n_roots": len(nodes), "status": STUCK}
    if carried is not None:
        from . import carry as CY
        asg, taken = carried
        sizes = CY.table_sizes_ck(nodes, asg)

        def compile_(probes):
            if not probes:
                return CY.compile_eval_ck(nodes, asg, sizes)
            return CY.compile_census_ck(nodes, asg, probes, sizes)
    else:
        def compile_(probes):
            return CS._compile(nodes, probes, form)
    if len(nodes) > 1 and refuted(nodes):
        out["status"] = CS.REFUTED
        return out
    if len(nodes) > CS.MAX_ROOTS:
        out.update(status=CS.UNSUPPORTED,
                   why="%d constraints (at most %d)" % (len(nodes), CS.MAX_ROOTS))
        return out
    # (built before the mask: a program's schedule follows the node ids, and a
    # wide mask leaves the compiler's spill budget little room)
    trees = distance_trees(nodes) if scored in ("tree", "aim", "bound", "uf", "sum") else None
    apps, uprobes = uf_probes(trees) if scored in ("uf", "sum") else ([], [])
    sprobes = sum_probes(trees) if scored == "sum" else []
    summed = False                                       # compiled with the side rows
    resid, table = residuals(nodes) if scored else ([], flat_table(len(nodes)))
    n_amask = 0
    try:
        ground = M._ground_value(compile_(()))
        if ground is not None:
            out["status"] = CS.GROUND_TRUE if ground else CS.GROUND_FALSE
            return out
        masked = compile_(CS.mask_probes(nodes))
        if trees is not None:
            # the atom mask and the trees' residuals; else the table's, below
            extra = CS.mask_probes(trees.atom_nodes) + trees.probes
            with_trees = None
            if scored == "sum":
                # the side rows after the residuals, then the arguments
                try:
                    with_trees = compile_(CS.mask_probes(nodes) + extra + sprobes + uprobes)
                except Unsupported:
                    with_trees = None
                if with_trees is None or with_trees.n_user_probes != \
                        masked.n_user_probes + len(extra) + len(sprobes) + len(uprobes):
                    with_trees, sprobes = None, []
                else:
                    summed = True
            if apps and with_trees is None:
                # the arguments of the UF slots after the residuals
                try:
                    with_trees = compile_(CS.mask_probes(nodes) + extra + uprobes)
                except Unsupported:
                    with_trees = None
                if with_trees is None or with_trees.n_user_probes != \
                        masked.n_user_probes + len(extra) + len(uprobes):
                    with_trees, apps, uprobes = None, [], []
            try:
                if with_trees is None:
                    with_trees = compile_(CS.mask_probes(nodes) + extra)
            except Unsupported:
                with_trees = None
            if with_trees is not None and with_trees.n_user_probes == \
                    masked.n_user_probes + len(extra) + len(sprobes) + len(uprobes):
                masked, resid, n_amask = with_trees, trees.probes, CS.n_mask_probes(trees.n_atoms)
            else:
                trees, apps, uprobes, sprobes, summed = None, [], [], [], False
        if resid and trees is None:
            # residuals the compiler folds or cannot place: the walkers rank by
            # the count alone
            try:
                with_resid = compile_(CS.mask_probes(nodes) + resid)
            except Unsupported:
                with_resid = None
            if with_resid is not None and \
                    with_resid.n_user_probes == masked.n_user_probes + len(resid):
                masked = with_resid
            else:
                resid, table = [], flat_table(len(nodes))
    except Unsupported as e:
        out.update(status=CS.UNSUPPORTED, why=str(e))
        return out
    n_mask = CS.n_mask_probes(len(nodes))
    aims = aim_table(trees, masked) if scored in ("aim", "bound", "uf", "sum") and \
        trees is not None else None
    bounds = bound_table(nodes, trees, masked) if scored in ("bound", "uf", "sum") and \
        trees is not None else None
    ufs = no_slots = sums = None
    if summed:
        sbounds, sufs, sums = sum_table(nodes, trees, masked, apps)
        if len(sbounds):
            bounds, ufs = sbounds, sufs
        else:
            sums = None
    if apps and sums is None:
        ubounds, ufs = uf_table(nodes, trees, masked, apps)
        if has_slot_piece(ubounds):
            bounds = ubounds
        else:
            ufs, no_slots = None, ufs
    if bounds is not None and not bounds.n_order and ufs is None:
        bounds = None
    if scored == "sum":
        out["sums"] = sums if sums is not None else no_sums(len(bounds) if bounds is not None else 0)
    if scored in ("uf", "sum"):
        out["ufs"] = ufs if ufs is not None else no_slots if no_slots is not None else no_ufs()
    if scored in ("bound", "uf", "sum"):
        out["bounds"] = bounds if bounds is not None else (
            bounds_of_aims(aims if aims is not None else no_aims(), len(nodes),
                           trees.n_atoms if trees is not None else 0))
    if scored:
        out["scoring"] = ("sum" if sums is not None and sums.n_linear else
                          "uf" if ufs is not None and (sums is None or has_slot_piece(bounds))
                          else "bound" if sums is not None and bounds.n_order else
                          "aim" if sums is not None else
                          "uf" if ufs is not None else "bound" if bounds is not None else
                          "aim" if aims is not None and len(aims) else
                          "tree" if trees is not None else "table" if resid else "count")
    if scored in ("aim", "bound", "uf", "sum"):
        out["aims"] = aims if aims is not None else no_aims()
        out["program"] = masked                          # what the table's leaves index
    if masked.n_user_probes != n_mask + n_amask + len(resid) + len(sprobes) + len(uprobes):
        out["status"] = CS.DEAD if masked.n_user_probes == 0 else CS.UNSUPPORTED
        out["why"] = "%d mask probes compiled to %d" % (n_mask, masked.n_user_probes)
        return out
    if not len(masked.leaves):
        out.update(status=CS.UNSUPPORTED, why="no leaf to move")
        return out
    eng = get_engine(device, nreg=masked.nreg)
    if carried is not None:
        gens = M.search_leafgen(masked)                  # as the carry loads its programs
        try:
            pin_rows, ladder = CY.rung_masks(masked, asg, *CY.split_nodes(nodes, taken))
        except ValueError as e:
            out.update(status=CS.UNSUPPORTED, why=str(e))
            return out
        keep = CY.distinct(ladder)
    else:
        gens = CS._leafgen(masked, form)
    view = eng.load(CS.census_view(masked, n_mask), gens, prog_seed=0)
    full = eng.load(masked, gens, prog_seed=0)
    if carried is not None:
        # the ladder's columns censused per rung; the starts are picked on the
        # device (carry.starts_ref) and their rows come with them
        free = [CY.n_free(masked, ladder[r]) for r in keep]
        cs, col, fails, rows = yield _CarryCensusJob(eng, view, pin_rows, ladder[keep], len(nodes),
                                                    walkers, any(free))
        out["census"], out["rungs"] = cs, keep
        picks = [int(v) for v in col]
        best_nfail = int(fails[0])
        out["start"] = {"col": picks[0], "rung": keep[picks[0] // max(1, cs[0].n_cand)],
                        "nfail": best_nfail}
        rows = list(rows)
    else:
        c = yield _CensusJob(eng, view, len(nodes), n_cand)
        out["census"] = c
        if not c.n_cand:
            return out
        # the starts, picked on the host: the best candidate, then the sole
        # blockers' candidates in rank order, padded with the best
        picks = [c.best_index]
        if c.best_nfail and scored:
            for k in c.blockers():
                if c.sole_index[k] >= 0 and int(c.sole_index[k]) not in picks:
                    picks.append(int(c.sole_index[k]))
            picks = (picks + [c.best_index] * walkers)[:walkers]
        rows = yield _WitnessJob(eng, full, picks)
        out["start"] = {"index": c.best_index, "nfail": c.best_nfail}
        best_nfail = c.best_nfail
    leaves = rows[0]
    out["repair"] = None
    seed = M.SEARCH_SEED if seed is None else seed
    if best_nfail and scored:
        starts = np.stack(rows)
        wide = eng.load(CS.census_view(masked, n_mask + n_amask + len(resid)), gens, prog_seed=0)
        n = len(nodes)
        if trees is not None and sums is not None:
            # the side rows after the residuals, then the U rows: the
            # arguments, then the kept keys
            wide = eng.load(uf_view(masked, n_mask + n_amask + len(resid) + len(sprobes) +
                                    ufs.n_arg_rows, ufs.keep), gens, prog_seed=0)
            rung, job = "sum", (wide, starts, n, trees, bounds, ufs, sums, seed)
        elif trees is not None and ufs is not None:
            # the U rows after the residuals: the arguments, then the kept keys
            wide = eng.load(uf_view(masked, n_mask + n_amask + len(resid) + ufs.n_arg_rows,
                                    ufs.keep), gens, prog_seed=0)
            rung, job = "uf", (wide, starts, n, trees, bounds, ufs, no_sums(len(bounds)), seed)
        elif trees is not None and bounds is not None:
            rung, job = "bound", (wide, starts, n, trees, bounds, no_ufs(),
                                  no_sums(len(bounds)), seed)
        elif trees is not None and aims is not None and len(aims):
            xor = bounds_of_aims(aims, n, trees.n_atoms)
            rung, job = "aim", (wide, starts, n, trees, xor, no_ufs(), no_sums(len(xor)), seed)
        elif trees is not None:
            rung, job = "tree", (wide, starts, n, trees,
                                 bounds_of_aims(no_aims(), n, trees.n_atoms), no_ufs(),
                                 no_sums(0), seed)
        if trees is not None:
            res = yield _TreeWalk(eng, rung, job, lanes, max_rounds, sync_every)
            out["trees"] = trees
        else:
            res = eng.walk(wide, starts, len(nodes), table, len(resid), seed, lanes, max_rounds,
                           sync_every)
        out.update(starts=picks, repair=res, table=table)
        if res.nfail[res.winner]:
            # which roots the winner still fails (one lane of the full program)
            _, probes = eng.eval(full, np.ascontiguousarray(res.leaves[res.winner][:, :, None]),
                                 want_probes=True)
            holds = CS.mask_bits(probes[:n_mask], len(nodes))[0]
            out["failing"] = [int(k) for k in np.flatnonzero(~holds)]
            if trees is not None and trees.n_atoms:
                # per atom: does it hold on the winner, and how far is it if not
                first = n_mask + n_amask
                abits = CS.mask_bits(probes[n_mask:first], trees.n_atoms)[0]
                # (lane i fails atom i alone, the atoms scored as simple roots)
                dist = _tree_score_bits(~np.eye(trees.n_atoms, dtype=bool), None, np.repeat(
                    probes[first:first + len(resid)], trees.n_atoms, axis=2),
                    simple_trees(trees.atoms))[1]
                out["atom_state"] = [(bool(h), 0 if h else int(d)) for h, d in zip(abits, dist)]
            return out
        leaves = res.leaves[res.winner]
    elif best_nfail:
        res = eng.repair(view, leaves, len(nodes), seed, lanes, max_rounds, sync_every)
        out["repair"] = res
        if res.nfail:
            return out
        leaves = res.leaves
    root, probes = eng.eval(full, np.ascontiguousarray(leaves[:, :, None]), want_probes=True)
    holds = CS.mask_bits(probes[:n_mask], len(nodes))[0]
    if not (bool(root[0]) and holds.all()):
        out["why"] = "the fresh evaluation of the repaired leaves fails %d constraints" % (
            int((~holds).sum()))
        return out
    out["status"] = REPAIRED
    out["assignment"] = unpack(masked, leaves, probes[:, :, 0] if masked.solved else None)
    return out


def repair_groups(groups: Sequence[Sequence], n_cand: int = 1 << 16, form: str = "search",
                  lanes: int = 4096, max_rounds: int = 64, device: int = 0,
                  seed: Optional[int] = None, sync_every: int = 8, scored=False,
                  walkers: int = 1, max_bytes: Optional[int] = None) -> List[dict]:
    """``[repair_group(g, ...) for g in groups]`` with the launches of all
    groups batched: their censuses in one ``Engine.census_batch``, their
    starts in one ``Engine.batch_witness`` and their
    tree-scored walks in one ``Engine.walk_batch`` (``mg_walk_batch``,
    DESIGN.md §3.16) — one of each per register layout, should the groups'
    programs differ in it: every key of every dict is what
    :func:`repair_group` returns but ``census.kernel_ms`` and
    ``repair.kernel_ms``, the device times of the batches the group ran in.
    Every group is compiled and driven to its census, then to its starts,
    then the walks run together, then every group is finished, per group.
    Groups that end without a walk (refuted, ground, unsupported, dead,
    satisfied by the census) and groups that fall back to the table or the
    count run as :func:`repair_group` runs them."""
    from . import model as M
    runs = [_repair_steps(g, n_cand, form, lanes, max_rounds, device, seed, sync_every, scored,
                          walkers) for g in groups]
    out: List[Optional[dict]] = [None] * len(runs)
    waiting = {}

    def advance(i, value=None):
        try:
            waiting[i] = next(runs[i]) if value is None else runs[i].send(value)
        except StopIteration as done:
            waiting.pop(i, None)
            out[i] = done.value

    for i in range(len(runs)):
        advance(i)
    walked = set()
    while waiting:
        # every group is driven to the earliest hand-over point any group waits
        # at: all censuses, then all witnesses, then all walks
        stage = min(w.stage for w in waiting.values())
        engines = []
        for w in waiting.values():
            if w.stage == stage and not any(e is w.eng for e in engines):
                engines.append(w.eng)
        for eng in engines:
            idx = [i for i in waiting if waiting[i].stage == stage and waiting[i].eng is eng]
            if stage == _CensusJob.stage:
                results = eng.census_batch([waiting[i].job for i in idx], M.SEARCH_SEED, 0, n_cand)
            elif stage == _WitnessJob.stage:
                pairs = [q for i in idx for q in waiting[i].pairs]
                rows = [r for r, _ in eng.batch_witness(pairs, M.SEARCH_SEED, want_probes=False)]
                results, at = [], 0
                for i in idx:
                    results.append(rows[at:at + len(waiting[i].picks)])
                    at += len(waiting[i].picks)
            else:
                if walked & set(idx):
                    raise RuntimeError("a group asked for a second walk")
                walked |= set(idx)
                results = eng.walk_batch([waiting[i].job for i in idx], lanes, max_rounds,
                                         sync_every, max_bytes)
            for i, res in zip(idx, results):
                advance(i, res)
    return out


def repair_carried(items, lanes_carry: Optional[int] = None, walkers: Optional[int] = None,
                   lanes: int = 4096, max_rounds: int = 64, sync_every: int = 8, scored="sum",
                   max_bytes: Optional[int] = None, device: int = 0, seed: Optional[int] = None,
                   count=None) -> List[dict]:
    """The walk from a carried start of the groups
    ``items``, a list of ``(nodes, assignment, taken_keys)`` as
    ``carry.run_ladder`` takes them: every group is compiled as
    :func:`_repair_steps` does with ``carried`` set, the ladders of all groups
    of an engine are censused in ONE ``Engine.carry_census`` call at
    ``lanes_carry`` candidates per rung (default ``carry.CARRY_LANES``; 1 when
    no rung of any group has a free leaf) and ``walkers`` start columns
    (default ``carry.CARRY_WALKERS``), the groups whose start 0 still fails a
    root walk together in one ``Engine.walk_batch`` and every group is finished
    by the fresh evaluation of the full masked program.  Per group the dict of
    :func:`repair_group` with ``census`` the per-rung list, ``rungs``,
    ``start`` and ``starts`` as :func:`_repair_steps` describes them, and
    ``miss_report`` (``carry.miss_report``) where a census ran.
    ``count(eng, launches)``: called after every launch sequence
    (``model._count_kernel``)."""
    from . import carry as CY
    from . import model as M
    lanes_carry = CY.CARRY_LANES if lanes_carry is None else lanes_carry
    walkers = CY.CARRY_WALKERS if walkers is None else walkers
    items = [(list(nodes), asg, taken) for nodes, asg, taken in items]
    runs = [_repair_steps(nodes, 0, "eval", lanes, max_rounds, device, seed, sync_every, scored,
                          walkers, carried=(asg, taken)) for nodes, asg, taken in items]
    out: List[Optional[dict]] = [None] * len(runs)
    waiting = {}

    def advance(i, value=None):
        try:
            waiting[i] = next(runs[i]) if value is None else runs[i].send(value)
        except StopIteration as done:
            waiting.pop(i, None)
            out[i] = done.value

    for i in range(len(runs)):
        advance(i)
    walked = set()
    while waiting:
        stage = min(w.stage for w in waiting.values())
        engines = []
        for w in waiting.values():
            if w.stage == stage and not any(e is w.eng for e in engines):
                engines.append(w.eng)
        for eng in engines:
            idx = [i for i in waiting if waiting[i].stage == stage and waiting[i].eng is eng]
            if stage == _CarryCensusJob.stage:
                jobs = [waiting[i].job for i in idx]
                width = max(1, int(lanes_carry)) if any(waiting[i].free for i in idx) else 1
                width = min(width, (1 << 20) // max(j[2].shape[0] for j in jobs))
                results = eng.carry_census(jobs, M.SEARCH_SEED, 0, width, walkers)
                if count:
                    # fill, interpreter, census, starts
                    count(eng, 4 * ((len(jobs) + 255) // 256))
            else:
                if walked & set(idx):
                    raise RuntimeError("a group asked for a second walk")
                walked |= set(idx)
                results = eng.walk_batch([waiting[i].job for i in idx], lanes, max_rounds,
                                         sync_every, max_bytes)
                if count:
                    # per round: mutate, interpreter, pick
                    count(eng, 3 * max(r.rounds for r in results))
            for i, res in zip(idx, results):
                advance(i, res)
    for (nodes, _, _), g in zip(items, out):
        if "rungs" in g:
            g["miss_report"] = CY.miss_report(nodes, g["census"], g["rungs"])
    return out


def repair(constraints: Sequence, **kw) -> dict:
    """:func:`repair_group` per independent group
    (``model.dependence_buckets``), each entry with the positions of its
    constraints in the caller's list (``constraints``); ``model`` is the
    joined assignment when every group is ground-true or repaired, else None.
    Touches no memo, gate or statistic of the model module."""
    from . import census as CS
    from .assign import Assignment
    from .model import _merge, dependence_buckets
    nodes = list(constraints)
    where = {}
    for i, c in enumerate(nodes):
        where.setdefault(c.id, []).append(i)
    groups, parts, whole = [], [], True
    for b in dependence_buckets(nodes):
        g = repair_group(b, **kw)
        g["constraints"] = [where[c.id].pop(0) for c in b]
        groups.append(g)
        if g["status"] == REPAIRED:
            parts.append(g["assignment"])
        elif g["status"] == CS.GROUND_TRUE:
            parts.append(Assignment())
        else:
            whole = False
    return {"groups": groups, "model": _merge(parts) if whole else None}

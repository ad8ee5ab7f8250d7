"""Per-constraint verdict census of a missed search.

The search answers one bit per candidate: do all constraints hold?  When no
candidate of the range satisfies a query, the census says why: per
constraint, how often it holds, how often it is the first or the only one
that fails, how close the best candidate came, and which candidate that was.

The verdict mask is built from source-DAG nodes (:func:`mask_probes`) and
compiled as probes of the query's own program, so neither compiler, the IR
nor the interpreter changes; the reduction over the candidates runs on the
device (``mg_census``, ``csrc/mg_census.hip``) and :func:`reduce_masks` is
its specification.

Candidate indices are those of the MASKED program: adding the mask can add
the numerals 0 and 1 to the constant pool, and leaves without a pool of
their own draw from it.  The census view (:func:`census_view`) and the full
masked program run the same candidate stream; the plain program that
``get_model`` compiles may not, so an index reported here is regenerated on
the masked program only.
"""

from __future__ import annotations

import copy
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import irdefs as I
from .ir import Program, Unsupported, compile_constraints
from .smt import node as N

MAX_ROOTS = 1024          # mg_census: n_roots 1..1024
PROBE_BITS = 256


def mask_probes(constraints: Sequence[N.Node]) -> List[N.Node]:
    """The verdict mask of ``constraints`` as probe nodes: bit k % 256 of
    probe k // 256 is ``ite(c_k, 1bv1, 0bv1)``, concatenated high-first, so
    bit k of the mask is constraint k.  One probe per 256 constraints; a
    single constraint is its own one-bit probe."""
    cs = list(constraints)
    one, zero = N.bv_num(1, 1), N.bv_num(0, 1)
    out = []
    for i in range(0, len(cs), PROBE_BITS):
        bits = [N.ite(c, one, zero) for c in cs[i:i + PROBE_BITS]]
        out.append(N.concat(*reversed(bits)))
    return out


def n_mask_probes(n_roots: int) -> int:
    return (n_roots + PROBE_BITS - 1) // PROBE_BITS


def census_view(program: Program, n_mask: int) -> Program:
    """``program`` (compiled with its mask probes first) with every ``OUT``
    of another probe replaced by ``NOP`` and ``n_probes = n_mask``: a census
    launch writes the mask probes only (a search program also reports its
    derived leaves and table keys as probes, hundreds of them).  Leaves,
    constants and pools are kept, so the view runs the candidate stream of
    the full masked program.  For the census only: a witness is unpacked
    from the full program."""
    if not 1 <= n_mask <= program.n_probes:
        raise ValueError("n_mask %d outside the program's %d probes" % (n_mask, program.n_probes))
    code = np.array(program.code, dtype=np.uint32, copy=True)
    other = ((code[:, 0] & 0xFF) == I.OUT) & (code[:, 2] >= n_mask)
    code[other] = (I.NOP, 0, 0, 0)
    view = copy.copy(program)
    view.code = code
    view.n_probes = n_mask
    return view


def mask_bits(masks: np.ndarray, n_roots: int) -> np.ndarray:
    """(n, n_roots) bool verdicts from host mask probes (n_mask, 8, n) u32;
    bits at or above ``n_roots`` are dropped."""
    masks = np.ascontiguousarray(masks, dtype="<u4")
    n_mask, limbs, n = masks.shape
    if limbs != 8 or n_mask < n_mask_probes(n_roots):
        raise ValueError("masks must be (n_mask >= %d, 8, n)" % n_mask_probes(n_roots))
    rows = np.ascontiguousarray(masks.reshape(n_mask * 8, n).T)          # (n, words)
    bits = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")
    return bits[:, :n_roots].astype(bool)


@dataclass
class Census:
    """Verdict census of the candidates [first_index, first_index + n_cand)
    over ``n_roots`` constraints (arrays are int64, one entry per root unless
    noted)."""
    n_roots: int
    first_index: int
    n_cand: int
    pass_: np.ndarray          # candidates on which root k holds
    first_block: np.ndarray    # candidates whose lowest failing root is k
    sole_block: np.ndarray     # candidates on which root k is the only failing root
    sole_index: np.ndarray     # the smallest such candidate index, or -1
    nfail_hist: np.ndarray     # [f], f = 0..n_roots: candidates with f failing roots
    best_nfail: int            # min over candidates of (failing roots, index);
    best_index: int            # n_roots + 1 and -1 over an empty range
    kernel_ms: float = 0.0     # device time of the launches (not compared)

    @property
    def n_sat(self) -> int:
        return int(self.nfail_hist[0])

    @property
    def first_sat(self) -> int:
        """The smallest satisfying candidate index, or -1."""
        return self.best_index if self.best_nfail == 0 else -1

    def as_dict(self) -> dict:
        return {"n_roots": self.n_roots, "first_index": self.first_index, "n_cand": self.n_cand,
                "pass": [int(v) for v in self.pass_],
                "first_block": [int(v) for v in self.first_block],
                "sole_block": [int(v) for v in self.sole_block],
                "sole_index": [int(v) for v in self.sole_index],
                "nfail_hist": [int(v) for v in self.nfail_hist],
                "best_nfail": int(self.best_nfail), "best_index": int(self.best_index)}

    def __eq__(self, other):
        return isinstance(other, Census) and self.as_dict() == other.as_dict()

    def merge(self, other: "Census") -> "Census":
        """The census of two disjoint ranges of the same program."""
        if self.n_roots != other.n_roots:
            raise ValueError("censuses of %d and %d roots" % (self.n_roots, other.n_roots))
        a, b = self.sole_index, other.sole_index
        sole = np.where(a < 0, b, np.where(b < 0, a, np.minimum(a, b)))
        best = min((c.best_nfail, c.best_index) for c in (self, other) if c.n_cand) \
            if self.n_cand or other.n_cand else (self.n_roots + 1, -1)
        first = min([c.first_index for c in (self, other) if c.n_cand] or [self.first_index])
        return Census(self.n_roots, first, self.n_cand + other.n_cand, self.pass_ + other.pass_,
                      self.first_block + other.first_block, self.sole_block + other.sole_block,
                      sole, self.nfail_hist + other.nfail_hist, best[0], best[1],
                      self.kernel_ms + other.kernel_ms)

    def blockers(self) -> List[int]:
        """Roots that fail on some candidate, worst first: roots no candidate
        satisfies, then by ``sole_block`` (the only thing between a candidate
        and a model), then by ``first_block``."""
        ks = [k for k in range(self.n_roots) if self.pass_[k] < self.n_cand]
        return sorted(ks, key=lambda k: (self.pass_[k] != 0, -int(self.sole_block[k]),
                                         -int(self.first_block[k]), k))

    def check(self) -> None:
        """The identities every census keeps."""
        assert int(self.first_block.sum()) + self.n_sat == self.n_cand
        assert int(self.sole_block.sum()) == int(self.nfail_hist[1])
        assert (self.sole_block <= self.first_block).all()
        assert (self.first_block <= self.n_cand - self.pass_).all()
        assert int(self.nfail_hist.sum()) == self.n_cand


def reduce_bits(bits: np.ndarray, first_index: int) -> Census:
    """The census of (n, n_roots) bool verdicts of candidates first_index.."""
    bits = np.asarray(bits, dtype=bool)
    n, r = bits.shape
    fail = ~bits
    nfail = fail.sum(axis=1)
    lowest = np.argmax(fail, axis=1)                   # of rows with a failure
    failing = nfail > 0
    sole = nfail == 1
    idx = np.arange(n, dtype=np.int64) + first_index
    sole_index = np.full(r, -1, dtype=np.int64)
    for k in np.unique(lowest[sole]):
        sole_index[k] = idx[sole & (lowest == k)].min()
    if n:
        best_nfail = int(nfail.min())
        best_index = int(idx[np.argmax(nfail == best_nfail)])
    else:
        best_nfail, best_index = r + 1, -1
    return Census(r, first_index, n, bits.sum(axis=0).astype(np.int64),
                  np.bincount(lowest[failing], minlength=r).astype(np.int64),
                  np.bincount(lowest[sole], minlength=r).astype(np.int64), sole_index,
                  np.bincount(nfail, minlength=r + 1).astype(np.int64), best_nfail, best_index)


def pack_block(c: Census) -> np.ndarray:
    """The device counter block of a census (csrc/mg_census.h; include/mythgpu.h
    describes it above mg_carry_census): 5 n + 2 uint64 — pass, first_block,
    sole_block, nfail_hist (n + 1), sole_index (all ones: none), best = failing
    roots << 53 | offset from ``first_index`` (all ones over an empty range).
    mg_carry_census counts columns from 0, so there the offset is the index."""
    n = c.n_roots
    ones = np.uint64(2**64 - 1)
    sole = np.where(np.asarray(c.sole_index) < 0, ones,
                    np.asarray(c.sole_index).astype(np.uint64))
    best = ones if c.best_index < 0 else np.uint64((int(c.best_nfail) << 53) | int(c.best_index))
    return np.concatenate([np.asarray(c.pass_, dtype=np.uint64),
                           np.asarray(c.first_block, dtype=np.uint64),
                           np.asarray(c.sole_block, dtype=np.uint64),
                           np.asarray(c.nfail_hist, dtype=np.uint64)[:n + 1], sole,
                           np.array([best], dtype=np.uint64)])


def unpack_block(block: np.ndarray, n_roots: int, first_index: int, n_cand: int,
                 kernel_ms: float = 0.0) -> Census:
    """:func:`pack_block` backwards for a block whose indices are absolute
    (mg_carry_census: column numbers)."""
    n = n_roots
    b = np.asarray(block, dtype=np.uint64)
    ones = np.uint64(2**64 - 1)
    sole = b[4 * n + 1:5 * n + 1]
    sole_index = np.where(sole == ones, np.int64(-1), sole.astype(np.int64))
    best = int(b[5 * n + 1])
    best_nfail, best_index = (n + 1, -1) if best == 2**64 - 1 else \
        (best >> 53, best & ((1 << 53) - 1))
    return Census(n, first_index, n_cand, b[:n].astype(np.int64), b[n:2 * n].astype(np.int64),
                  b[2 * n:3 * n].astype(np.int64), sole_index, b[3 * n:4 * n + 1].astype(np.int64),
                  int(best_nfail), int(best_index), kernel_ms)


def reduce_masks(masks: np.ndarray, n_roots: int, first_index: int) -> Census:
    """Exactly the outputs of the census kernel, from host mask probes
    (n_mask, 8, n) u32 of candidates first_index ..: the kernel's
    specification."""
    return reduce_bits(mask_bits(masks, n_roots), first_index)


# ---------------------------------------------------------------------------
# explain a miss
# ---------------------------------------------------------------------------

REFUTED, GROUND_FALSE, GROUND_TRUE, DEAD, UNSUPPORTED, CENSUS = (
    "refuted", "ground-false", "ground-true", "construction-dead", "unsupported", "census")


def _compile(nodes, probes, form: str) -> Program:
    if form == "search":
        from .model import _compile_search_uncached          # (no search-program memo)
        return _compile_search_uncached(nodes, probes)
    return compile_constraints(nodes, probes)


def _leafgen(prog: Program, form: str):
    from .engine import default_leafgen
    from .model import search_leafgen
    return search_leafgen(prog) if form == "search" else default_leafgen(prog)


def _explain_prepare(nodes: Sequence[N.Node], form: str):
    """The host part of :func:`explain_group`: ``(out, job)`` with ``job`` None
    for a group that launches nothing (``out`` is then its whole entry), else
    ``(masked, plain, n_mask)``: the full masked program, the plain one and the
    number of mask probes."""
    from . import model as M
    from .refute import refuted
    out: dict = {"n_roots": len(nodes), "status": CENSUS}
    if len(nodes) > 1 and refuted(nodes):
        out["status"] = REFUTED
        return out, None
    if len(nodes) > MAX_ROOTS:
        out.update(status=UNSUPPORTED, why="%d constraints (at most %d)" % (len(nodes), MAX_ROOTS))
        return out, None
    try:
        plain = _compile(nodes, (), form)
        ground = M._ground_value(plain)
        if ground is not None:
            out["status"] = GROUND_TRUE if ground else GROUND_FALSE
            return out, None
        masked = _compile(nodes, mask_probes(nodes), form)
    except Unsupported as e:
        out.update(status=UNSUPPORTED, why=str(e))
        return out, None
    n_mask = n_mask_probes(len(nodes))
    if masked.n_user_probes != n_mask:
        # solve mode drops the probes when the construction meets a false
        # root: no model it builds can satisfy the group
        out["status"] = DEAD if masked.n_user_probes == 0 else UNSUPPORTED
        out["why"] = "%d mask probes compiled to %d" % (n_mask, masked.n_user_probes)
        return out, None
    return out, (masked, plain, n_mask)


def _explain_census(out: dict, job, c: "Census") -> None:
    masked, plain, _ = job
    out.update(census=c, blockers=c.blockers(), records=masked.n_ins,
               plain_records=plain.n_ins, plain_program=plain)


def _explain_best(out: dict, job, n_roots: int, leaves, probes) -> None:
    from .assign import unpack
    masked, _, n_mask = job
    c = out["census"]
    holds = mask_bits(probes[:n_mask, :, None], n_roots)[0]
    out["best"] = {"index": c.best_index, "nfail": c.best_nfail,
                   "failing": [int(k) for k in np.flatnonzero(~holds)],
                   "assignment": unpack(masked, leaves, probes if masked.solved else None)}


def explain_group(nodes: Sequence[N.Node], n_cand: int = 1 << 16, form: str = "search",
                  device: int = 0, chunk: int = 0) -> dict:
    """The report entry of ONE independent group (root k = ``nodes[k]``):
    ``status`` and, for a group that was launched, its ``census``, ranked
    ``blockers`` and the ``best`` candidate (index, failing roots, failing
    root indices, assignment regenerated on the full masked program)."""
    from . import model as M
    from .engine import get_engine
    nodes = list(nodes)
    out, job = _explain_prepare(nodes, form)
    if job is None:
        return out
    masked, _, n_mask = job
    eng = get_engine(device, nreg=masked.nreg)
    gens = _leafgen(masked, form)
    lp = eng.load(census_view(masked, n_mask), gens, prog_seed=0)
    c = eng.census(lp, M.SEARCH_SEED, 0, n_cand, len(nodes), 0, chunk)
    _explain_census(out, job, c)
    if c.n_cand:
        full = eng.load(masked, gens, prog_seed=0)
        leaves, probes = eng.witness(full, M.SEARCH_SEED, c.best_index)
        _explain_best(out, job, len(nodes), leaves, probes)
    return out


def explain_groups(groups: Sequence[Sequence[N.Node]], n_cand: int = 1 << 16,
                   form: str = "search", device: int = 0, chunk: int = 0) -> List[dict]:
    """``[explain_group(g, ...) for g in groups]`` with the launches of all
    groups batched: the censuses of the launched groups run
    in one ``Engine.census_batch`` and their best candidates are regenerated
    in one ``Engine.batch_witness`` — one of each per register layout, should
    the groups' programs differ in it.  Every key of every entry is what
    :func:`explain_group` returns but ``census.kernel_ms``, the device time of
    the batch the group's census ran in."""
    from . import model as M
    from .engine import get_engine
    groups = [list(g) for g in groups]
    prepared = [_explain_prepare(g, form) for g in groups]
    outs = [out for out, _ in prepared]
    by_engine: Dict[int, list] = {}
    for i, (_, job) in enumerate(prepared):
        if job is not None:
            eng = get_engine(device, nreg=job[0].nreg)
            by_engine.setdefault(id(eng), [eng, []])[1].append(i)
    for eng, idx in by_engine.values():
        gens = {i: _leafgen(prepared[i][1][0], form) for i in idx}
        views = [eng.load(census_view(prepared[i][1][0], prepared[i][1][2]), gens[i], prog_seed=0)
                 for i in idx]
        cs = eng.census_batch([(lp, len(groups[i]), 0) for lp, i in zip(views, idx)],
                              M.SEARCH_SEED, 0, n_cand, chunk)
        for i, c in zip(idx, cs):
            _explain_census(outs[i], prepared[i][1], c)
        best = [i for i in idx if outs[i]["census"].n_cand]
        fulls = [eng.load(prepared[i][1][0], gens[i], prog_seed=0) for i in best]
        wit = eng.batch_witness([(lp, outs[i]["census"].best_index) for lp, i in zip(fulls, best)],
                                M.SEARCH_SEED)
        for i, (leaves, probes) in zip(best, wit):
            _explain_best(outs[i], prepared[i][1], len(groups[i]), leaves, probes)
    return outs


def explain(constraints: Sequence[N.Node], n_cand: int = 1 << 16, form: str = "search",
            device: int = 0, chunk: int = 0) -> dict:
    """Why no candidate satisfies ``constraints``: one entry per independent
    group (``model.dependence_buckets``), root indices mapped back to the
    positions of the constraints in the caller's list (``constraints``,
    ``blockers``, ``best["failing"]``).  A group the host refutes, one the
    compiler folds to a constant, one whose model construction died and one
    the mask makes uncompilable say so (``status``) and launch nothing; every
    other group gets a :class:`Census` over ``n_cand`` candidates from index
    0 of the group's masked program (``form``: "search", the program
    ``get_model`` searches, or "eval", the plain form with the default
    generator).  Touches no memo, gate or statistic of the model module."""
    if form not in ("search", "eval"):
        raise ValueError("form must be 'search' or 'eval'")
    from .model import dependence_buckets
    nodes = list(constraints)
    where: Dict[int, List[int]] = {}
    for i, c in enumerate(nodes):
        where.setdefault(c.id, []).append(i)
    groups = []
    buckets = [list(b) for b in dependence_buckets(nodes)]
    for b, g in zip(buckets, explain_groups(buckets, n_cand, form, device, chunk)):
        pos = [where[c.id].pop(0) for c in b]
        g["constraints"] = pos
        if "blockers" in g:
            g["blockers"] = [pos[k] for k in g["blockers"]]
        if "best" in g:
            g["best"]["failing"] = [pos[k] for k in g["best"]["failing"]]
        groups.append(g)
    return {"n_cand": n_cand, "form": form, "groups": groups}

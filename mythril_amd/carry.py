"""Witness carry: a group's model reused on the groups that
extend it.

LASER builds its queries along a path: it appends one JUMPI condition, asks
``is_possible``, appends the next.  The group-miss memo of ``model.py`` answers
a group that repeats or extends a MISSED group; this module does the same for
hits.  A group that found a witness is remembered (:class:`HitMemo`); an exact
repeat is answered from the memo, and a group that properly extends remembered
groups is evaluated ONCE under their witnesses: the extended group is compiled
in eval form, the leaves the carried assignment interprets are pinned to its
values (:func:`pins`), the leaves of fresh symbols come from the device
generator, and ``Engine.carry_batch`` runs every such job of a query — or of a
whole ``batch_is_possible`` call — in one launch sequence.

The carry never concludes UNSAT: a group it misses is searched as before, and a
carried witness is accepted by the same rule as any other (``model._accept``).
Opt-in: ``MYTHRIL_GPU_CARRY=1``.

``MYTHRIL_GPU_CARRY=2`` runs the pin ladder instead: the
extended group is compiled in eval form WITH constant keys
(:func:`compile_eval_ck`), several pin sets — all, read, new (:func:`rungs`) —
are tried strictest first, and ``Engine.carry_ladder`` evaluates every rung of
every job in the same three launches (:func:`run_ladder`).

``MYTHRIL_GPU_CARRY=4`` gives the ladder's rungs their own pin rows (DESIGN.md
§3.21): the remembered subsets :func:`union` skips because they share a name
with one taken before them become further pin sets (:func:`plan_sets`), every
rung of every set is a block of columns of the one compiled group
(:func:`rungs_sets`), and ``Engine.carry_ladder_sets`` evaluates them in the
ladder's three launches (:func:`run_sets`).

``MYTHRIL_GPU_CARRY=5`` is the delta carry: only the
constraints an extension ADDS are compiled and evaluated
(:func:`delta_job`), on the two rungs that move no leaf the remembered
constraints read, so their roots hold as they did; a hit's column is written
into the remembered witness (:func:`merge_delta`), and
``Engine.carry_ladder`` runs every such job of a call (:func:`run_delta`).
"""

from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .assign import Assignment, leaf_values, lookup, unpack
from .ir import Program, compile_constraints, scan_const_keys

# candidates of a job with at least one free leaf (MYTHRIL_GPU_CARRY_LANES);
# a job with no free leaf runs one.  256 is one block of the interpreter and
# four groups of the generator's classes; DESIGN.md §7 records how the hit
# rate on extensions moves with it
CARRY_LANES = 256
DEFAULT_ENTRIES = 2            # compile_constraints' default table size
# the largest carried table an extension is evaluated with
# (MYTHRIL_GPU_CARRY_MAX_ENTRIES).  The eval form lowers a read of a table of n
# entries to n compare-and-select steps, so its size and compile time grow with
# every read times n; a witness that went through the ABI presets holds
# calldata tables of 68 constant-keyed entries, at which the eval form of a path
# group measured 2400 - 3700 records and 12 - 24 ms of compile, several times
# the solve-mode compile and search the carry is there to save (DESIGN.md §7
# round 16).  16 is eight times the default: what a few transactions' storage
# and balance tables reach, below any calldata table that carries presets.
MAX_ENTRIES = 16
EVAL_CACHE_SIZE = 2048


class HitMemo:
    """Group key (``model._group_key``: the frozenset of a group's node ids)
    -> the Assignment that satisfied the group.  Bounded (``size`` entries,
    oldest dropped) and indexed by each key's minimum id, as the group-miss
    memo is: a subset of a key that contains the key's minimum has it as its
    own minimum, and one that does not is found under the id that is.  An
    entry never expires: node ids are hash-consed and never reused, so a
    group's witness is a function of its key."""

    def __init__(self, size: int):
        self.size = size
        self.hits: Dict[frozenset, Assignment] = {}
        self.progs: Dict[frozenset, Program] = {}     # a program of the group (table sizes)
        self.index: Dict[int, List[frozenset]] = {}
        self.seq: Dict[frozenset, int] = {}
        self._n = 0

    def note(self, key: frozenset, asg: Assignment, prog: Optional[Program] = None) -> None:
        if not key or asg is None:
            return
        if key not in self.hits:
            while len(self.hits) >= max(1, self.size):
                self._drop(next(iter(self.hits)))
            self.index.setdefault(min(key), []).append(key)
        self.hits[key] = asg
        self._n += 1
        self.seq[key] = self._n
        if prog is not None:
            self.progs[key] = prog

    def _drop(self, old: frozenset) -> None:
        del self.hits[old]
        self.seq.pop(old, None)
        self.progs.pop(old, None)
        lst = self.index.get(min(old), [])
        if old in lst:
            lst.remove(old)
        if not lst:
            self.index.pop(min(old), None)

    def clear(self) -> None:
        self.hits.clear()
        self.progs.clear()
        self.index.clear()
        self.seq.clear()

    def subsets(self, key: frozenset) -> List[frozenset]:
        """The remembered proper subsets of ``key``, largest first and newest
        first among equals."""
        out = []
        for c in key:
            for m in self.index.get(c, ()):
                if len(m) < len(key) and m <= key:
                    out.append(m)
        out.sort(key=lambda m: (-len(m), -self.seq.get(m, 0)))
        return out

    def __len__(self):
        return len(self.hits)


def _names(a: Assignment) -> set:
    return set(a.vars) | set(a.arrays) | set(a.funcs)


def union(parts: Sequence[Assignment]) -> Tuple[Assignment, List[int]]:
    """The pin set of an extension: the assignments of ``parts`` in order,
    skipping any that interprets a name one taken before it interprets (two
    remembered groups that share a symbol may disagree on it; each was a
    witness only as a whole).  Returns the union and the indices taken."""
    out, taken, seen = Assignment(), [], set()
    for i, a in enumerate(parts):
        names = _names(a)
        if names & seen:
            continue
        seen |= names
        out.vars.update(a.vars)
        out.arrays.update(a.arrays)
        out.funcs.update(a.funcs)
        taken.append(i)
    return out, taken


def plan(key: frozenset, memo: HitMemo):
    """What the memo offers a group, a pure function of (key, memo):
    ``("exact", assignment)`` for a remembered key, ``("extend", assignment,
    subset keys taken)`` when remembered proper subsets give a pin set that
    interprets at least one name, else None."""
    hit = memo.hits.get(key)
    if hit is not None:
        return ("exact", hit)
    subs = memo.subsets(key)
    if not subs:
        return None
    asg, taken = union([memo.hits[m] for m in subs])
    if not _names(asg):
        return None
    return ("extend", asg, [subs[i] for i in taken])


def table_sizes(asg: Assignment, default: int = DEFAULT_ENTRIES) -> Dict[str, int]:
    """``table_sizes`` for the eval form of a group evaluated under ``asg``:
    the maximum of the default and the carried tables' entry counts (as
    ``Model.eval_node`` sizes its programs)."""
    return {name: max(default, len(entries))
            for name, (entries, _) in list(asg.arrays.items()) + list(asg.funcs.items())}


_EVAL_CACHE: "OrderedDict[tuple, Program]" = OrderedDict()


def clear() -> None:
    _EVAL_CACHE.clear()
    _PARENT_CACHE.clear()


def compile_eval(nodes, asg: Assignment) -> Program:
    """The eval form of a group to be evaluated under ``asg``: EVERY constraint
    of the group, so a carried hit rests on the same evidence as a search hit —
    every root true on the device.  Cached by node ids and table sizes."""
    sizes = table_sizes(asg)
    key = (tuple(n.id for n in nodes), tuple(sorted(sizes.items())))
    prog = _EVAL_CACHE.get(key)
    if prog is not None:
        _EVAL_CACHE.move_to_end(key)
        return prog
    prog = compile_constraints(nodes, solve=False, leaf_pools=True, table_sizes=sizes or None)
    _EVAL_CACHE[key] = prog
    if len(_EVAL_CACHE) > EVAL_CACHE_SIZE:
        _EVAL_CACHE.popitem(last=False)
    return prog


def pinned(leaf, asg: Assignment) -> bool:
    """A leaf is pinned iff the carried assignment interprets its source."""
    if leaf.kind == "var":
        return leaf.source in asg.vars
    if leaf.kind == "aux":
        return False
    return leaf.source in asg.arrays or leaf.source in asg.funcs


def pins(program: Program, asg: Assignment) -> Tuple[np.ndarray, np.ndarray]:
    """``(mask, rows)`` of one carry job: bit l of ``mask`` ((n_leaves + 31) //
    32 uint32 words) is set iff ``asg`` interprets leaf l's source — a var in
    ``vars``, a table in ``arrays`` or ``funcs``; ``rows`` ((n_leaves, 8)
    uint32) holds what ``assign.leaf_values`` gives for the pinned leaves, per
    chunk and masked to the leaf's width, and zero for the free ones (leaves of
    fresh symbols: a new transaction's calldata, call value, sender)."""
    n = len(program.leaves)
    mask = np.zeros((n + 31) // 32, dtype=np.uint32)
    rows = np.zeros((n, 8), dtype=np.uint32)
    vals = leaf_values(program, asg) if n else []
    for l, (leaf, v) in enumerate(zip(program.leaves, vals)):
        if not pinned(leaf, asg):
            continue
        mask[l >> 5] |= np.uint32(1 << (l & 31))
        rows[l] = np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u4")
    return mask, rows


def n_free(program: Program, mask: np.ndarray) -> int:
    n = len(program.leaves)
    return n - sum(bin(int(w)).count("1") for w in mask)


# ---------------------------------------------------------------------------
# The pin ladder (MYTHRIL_GPU_CARRY=2): the eval form with
# constant keys and several pin sets per job, strictest first
# ---------------------------------------------------------------------------

MAX_RUNGS = 8                  # include/mythgpu.h MG_CARRY_MAX_RUNGS
RUNG_NAMES = ("all", "read", "new")


def table_sizes_ck(nodes, asg: Assignment, default: int = DEFAULT_ENTRIES) -> Dict[str, int]:
    """``table_sizes`` for the constant-keyed eval form of ``nodes`` evaluated
    under ``asg``: per carried table the maximum of the default and the number
    of its entries whose key is not a constant key the nodes read the table at
    (``scan_const_keys``) — the entries ``assign.leaf_values`` leaves in the
    leaf-keyed part; those at constant keys are served by ``cval`` leaves.  A
    table the nodes read at constant keys only has no leaf-keyed part at all —
    every read is a ``cval`` leaf, no ``key`` or ``val`` leaf exists and no
    other entry of the witness can be met — so it keeps the default whatever
    the witness holds (a calldata witness of 68 entries read at bytes 0..4)."""
    sym: Dict[str, int] = {}
    ck = scan_const_keys(nodes, sym_counts=sym)
    out = {}
    for name, (entries, _) in list(asg.arrays.items()) + list(asg.funcs.items()):
        keys = set(ck.get(name, ()))
        rest = sum(1 for k, _ in entries if k not in keys) if sym.get(name) else 0
        out[name] = max(default, rest)
    return out


def compile_eval_ck(nodes, asg: Assignment, sizes: Optional[Dict[str, int]] = None) -> Program:
    """:func:`compile_eval` with constant keys: every numeral-keyed read is a
    ``cval`` leaf of its own, so a carried table costs its remaining entries
    only (``sizes``: :func:`table_sizes_ck`, computed when not given).  Cached
    with the plain form, under a key that names the form."""
    sizes = table_sizes_ck(nodes, asg) if sizes is None else sizes
    key = ("ck", tuple(n.id for n in nodes), tuple(sorted(sizes.items())))
    prog = _EVAL_CACHE.get(key)
    if prog is not None:
        _EVAL_CACHE.move_to_end(key)
        return prog
    prog = compile_constraints(nodes, solve=False, leaf_pools=True, const_keys=True,
                               table_sizes=sizes or None)
    _EVAL_CACHE[key] = prog
    if len(_EVAL_CACHE) > EVAL_CACHE_SIZE:
        _EVAL_CACHE.popitem(last=False)
    return prog


def _symbol_names(nodes) -> set:
    from .smt.node import topo_order
    return {n.params[0] for n in topo_order(list(nodes)) if n.op in ("var", "array", "apply")}


def rung_masks(program: Program, asg: Assignment, parent_nodes, new_nodes):
    """``(rows, ladder)`` of one ladder job: ``rows`` ((n_leaves, 8) uint32) as
    :func:`pins` gives them — every leaf the strictest rung pins holds its
    carried value, so one row set serves all rungs — and ``ladder``
    ((len(RUNG_NAMES), (n_leaves + 31) // 32) uint32), the mask of every rung
    of ``RUNG_NAMES``, strictest first:

    * "all": the rule of :func:`pins`, every leaf whose source ``asg``
      interprets.
    * "read": as "all", but a ``cval`` leaf at a key the parent never read its
      table at (``scan_const_keys(parent_nodes)``) is free: that entry of the
      witness was a don't-care.  ``key``, ``val`` and ``else`` leaves and vars
      stay pinned, and a table the parent reads at a symbolic key without
      ``scan_const_keys`` listing it (no numeral key, or too many symbolic
      links) frees nothing: any entry may have been what that read met.
    * "new": as "read", and every leaf whose source occurs in ``new_nodes``
      is free.

    ``parent_nodes``: the group's nodes of the remembered subsets the pin set
    was taken from (``plan``'s keys); ``new_nodes``: the rest."""
    n = len(program.leaves)
    words = (n + 31) // 32
    rows = np.zeros((n, 8), dtype=np.uint32)
    ladder = np.zeros((len(RUNG_NAMES), words), dtype=np.uint32)
    sym: Dict[str, int] = {}
    read = scan_const_keys(parent_nodes, sym_counts=sym)
    closed = {name for name, k in sym.items() if k and name not in read}
    fresh = _symbol_names(new_nodes)
    vals = leaf_values(program, asg) if n else []
    for l, (leaf, v) in enumerate(zip(program.leaves, vals)):
        if not pinned(leaf, asg):
            continue
        rows[l] = np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u4")
        keep = [True, True, True]
        if leaf.kind == "cval" and leaf.source not in closed:
            key = program.table_ckeys[leaf.source][leaf.entry]
            keep[1] = key in read.get(leaf.source, ())
        keep[2] = keep[1] and leaf.source not in fresh
        for r in range(len(RUNG_NAMES)):
            if keep[r]:
                ladder[r, l >> 5] |= np.uint32(1 << (l & 31))
    return rows, ladder


def distinct(ladder: np.ndarray) -> List[int]:
    """The rows of ``ladder`` that differ from every row before them, in
    order, ``MAX_RUNGS`` at the most."""
    kept: List[int] = []
    for r in range(ladder.shape[0]):
        if not any(np.array_equal(ladder[r], ladder[k]) for k in kept):
            kept.append(r)
    return kept[:MAX_RUNGS]


def rungs(program: Program, asg: Assignment, parent_nodes, new_nodes):
    """``(rows, masks)`` of one ladder job: the rows and the distinct masks of
    :func:`rung_masks`, strictest first."""
    rows, ladder = rung_masks(program, asg, parent_nodes, new_nodes)
    return rows, ladder[distinct(ladder)]


def split_nodes(nodes, taken_keys):
    """``(parent_nodes, new_nodes)`` of a group: the nodes whose ids lie in the
    subset keys :func:`plan` reports as taken, and the rest."""
    ids = set().union(*taken_keys) if taken_keys else set()
    return [n for n in nodes if n.id in ids], [n for n in nodes if n.id not in ids]


def run_ladder(eng, items, seed: int, leafgen, lanes: Optional[int] = None, phase=None):
    """:func:`run` on the pin ladder: one ``Engine.carry_ladder`` call for
    ``items``, a list of ``(nodes, assignment, taken_keys)`` (``plan``'s third
    element).  Per item ``(assignment, program, candidates, rung)`` — the
    witness (None on a miss), the constant-keyed eval form, the candidates the
    job ran over all its rungs and the index in ``RUNG_NAMES`` of the rung
    that hit (-1 on a miss) — or None where the group has no eval form.  A
    rung without a free leaf is one candidate; a batch none of whose rungs has
    one runs one lane."""
    import contextlib
    from .ir import Unsupported
    phase = phase or (lambda name: contextlib.nullcontext())
    lanes = CARRY_LANES if lanes is None else lanes
    jobs, progs, free, kept, where = [], [], [], [], []
    with phase("compile"):
        for k, (nodes, asg, taken) in enumerate(items):
            try:
                prog = compile_eval_ck(nodes, asg)
                rows, ladder = rung_masks(prog, asg, *split_nodes(nodes, taken))
            except (Unsupported, ValueError):
                continue
            keep = distinct(ladder)
            progs.append(prog)
            kept.append(keep)
            free.append([n_free(prog, ladder[r]) for r in keep])
            jobs.append((prog, rows, ladder[keep]))
            where.append(k)
    out: List = [None] * len(items)
    if not jobs:
        return out
    width = max(1, int(lanes)) if any(any(f) for f in free) else 1
    width = min(width, (1 << 20) // max(len(keep) for keep in kept))   # the call's column cap
    with phase("load"):
        loaded = [(eng.load(p, leafgen(p), prog_seed=0), r, m) for p, r, m in jobs]
    with phase("search"):
        res = eng.carry_ladder(loaded, seed, 0, width)
        for k, prog, f, keep, (first, rung, leaves) in zip(where, progs, free, kept, res):
            out[k] = (unpack(prog, leaves) if first >= 0 else None, prog,
                      sum(width if x else 1 for x in f), keep[rung] if first >= 0 else -1)
    return out


# ---------------------------------------------------------------------------
# The delta carry (MYTHRIL_GPU_CARRY=5): only the constraints
# an extension adds are compiled and evaluated, on the rungs that keep every
# leaf the parent reads
# ---------------------------------------------------------------------------

DELTA_RUNG_NAMES = ("all", "read")
_PARENT_CACHE: "OrderedDict[frozenset, tuple]" = OrderedDict()


def _parent_reads(parent_nodes, taken_keys):
    """``(symbol names, numeral keys read per table, symbolic reads per
    table)`` of a delta job's parent, cached by the subset keys taken: the
    children of one JUMPI, and the extensions after them, share their parent,
    and node ids are never reused."""
    key = frozenset(taken_keys)
    got = _PARENT_CACHE.get(key)
    if got is not None:
        _PARENT_CACHE.move_to_end(key)
        return got
    sym: Dict[str, int] = {}
    read = scan_const_keys(parent_nodes, sym_counts=sym)
    got = _PARENT_CACHE[key] = (_symbol_names(parent_nodes), read, sym)
    if len(_PARENT_CACHE) > EVAL_CACHE_SIZE:
        _PARENT_CACHE.popitem(last=False)
    return got


def delta_job(nodes, asg: Assignment, taken_keys):
    """``(program, rows, ladder)`` of one delta job: the constant-keyed eval
    form of the NEW nodes of the group alone (:func:`split_nodes`), sized by
    ``table_sizes_ck(new_nodes, asg)``; ``rows`` as :func:`pins` gives them;
    ``ladder`` ((2, words) uint32), the masks of ``DELTA_RUNG_NAMES``,
    strictest first:

    * "all": the rule of :func:`pins`.
    * "read" (read-strict): as "all", but a ``cval`` leaf is free when the
      parent reads its table at NO symbolic key (``scan_const_keys``'
      ``sym_counts``) and the leaf's key is not among the numeral keys the
      parent read.  :func:`rung_masks` frees such a leaf as soon as the scan
      lists the table, because the ladder evaluates the parent's roots again;
      the delta does not, so a symbolic read — which may have met any entry —
      keeps every entry.  Where the scan's key list is full (``CKEY_CAP``) it
      may have dropped a key the parent read: the table frees nothing.

    The parent's roots are not evaluated: they held under ``asg``, and neither
    rung moves a leaf they read.  That needs ``asg`` to speak for every symbol
    the two sides share, so ``ValueError`` is raised (with the reason) when a
    leaf of the program has a source the parent's nodes mention and ``asg``
    does not interpret — the delta would choose it freely and the parent's
    roots might not hold — and when the group has no new node."""
    from .ir import CKEY_CAP
    parent_nodes, new_nodes = split_nodes(nodes, taken_keys)
    if not new_nodes or not parent_nodes:
        raise ValueError("no delta: %d new and %d remembered constraints" % (
            len(new_nodes), len(parent_nodes)))
    program = compile_eval_ck(new_nodes, asg, table_sizes_ck(new_nodes, asg))
    shared, read, sym = _parent_reads(parent_nodes, taken_keys)
    for leaf in program.leaves:
        if leaf.kind != "aux" and leaf.source in shared and not pinned(leaf, asg):
            raise ValueError("the witness is silent about %s, which the remembered "
                             "constraints read" % leaf.source)
    mask, rows = pins(program, asg)
    ladder = np.stack([mask, mask.copy()])
    for l, leaf in enumerate(program.leaves):
        if leaf.kind != "cval" or not pinned(leaf, asg) or sym.get(leaf.source):
            continue
        keys = read.get(leaf.source, ())
        if len(keys) >= CKEY_CAP:
            continue
        if program.table_ckeys[leaf.source][leaf.entry] not in keys:
            ladder[1, l >> 5] &= ~np.uint32(1 << (l & 31))
    return program, rows, ladder


def _freed_keys(program: Program, asg: Assignment, mask: np.ndarray) -> Dict[str, List[int]]:
    """Per table ``asg`` interprets, the keys of the ``cval`` leaves of
    ``program`` that ``mask`` leaves free."""
    out: Dict[str, List[int]] = {}
    for l, leaf in enumerate(program.leaves):
        if leaf.kind == "cval" and pinned(leaf, asg) and not int(mask[l >> 5]) >> (l & 31) & 1:
            key = program.table_ckeys[leaf.source][leaf.entry]
            if key not in out.setdefault(leaf.source, []):
                out[leaf.source].append(key)
    return out


def merge_delta(asg: Assignment, program: Program, leaves: np.ndarray,
                mask: np.ndarray) -> Assignment:
    """The assignment of the whole group after a delta hit: a copy of ``asg``,
    with every var, array and function of ``unpack(program, leaves)`` that
    ``asg`` does not interpret, and — for the tables it does — exactly the
    entries at the keys of ``cval`` leaves that were free under ``mask``
    (:func:`delta_job`'s rung that hit): such an entry is written, in place of
    the don't-care entry the table held at that key if it held one.  Nothing
    else of a carried table changes (``model._merge`` replaces whole tables:
    the entries the parent's roots read would be lost)."""
    got = unpack(program, leaves)
    out = Assignment(asg.vars, asg.arrays, asg.funcs)
    for name, v in got.vars.items():
        out.vars.setdefault(name, v)
    for mine, theirs in ((out.arrays, got.arrays), (out.funcs, got.funcs)):
        for name, tab in theirs.items():
            if name not in out.arrays and name not in out.funcs:
                mine[name] = tab
    for name, keys in _freed_keys(program, asg, mask).items():
        mine = out.arrays if name in out.arrays else out.funcs
        entries, default = mine[name]
        new = got.table(name)
        mine[name] = ([(k, lookup(new, k)) for k in keys] +
                      [e for e in entries if e[0] not in keys], default)
    return out


def run_delta(eng, items, seed: int, leafgen, lanes: Optional[int] = None, phase=None):
    """:func:`run_ladder` on the delta: one ``Engine.carry_ladder`` call for the
    eligible ``items`` (``(nodes, assignment, taken_keys)``), every job the
    program of its new nodes alone (:func:`delta_job`).  Per item
    ``(assignment, program, candidates, rung)`` — on a hit the MERGED
    assignment of the whole group (:func:`merge_delta`) and the index in
    ``DELTA_RUNG_NAMES`` of the rung that hit, on a miss None and -1 —,
    ``("ineligible", reason)`` where :func:`delta_job` refuses, or None where
    the new nodes have no eval form.  A delta program that folds to a constant
    (``model._ground_value``) is answered without a launch, ``candidates`` 0:
    true is a hit on "all" with the witness as it is, false a miss.  The width
    rule and the column cap are :func:`run_ladder`'s."""
    import contextlib
    from .ir import Unsupported
    from .model import _ground_value
    phase = phase or (lambda name: contextlib.nullcontext())
    lanes = CARRY_LANES if lanes is None else lanes
    out: List = [None] * len(items)
    jobs, progs, free, kept, where = [], [], [], [], []
    with phase("compile"):
        for k, (nodes, asg, taken) in enumerate(items):
            try:
                prog, rows, ladder = delta_job(nodes, asg, taken)
            except Unsupported:
                continue
            except ValueError as e:
                out[k] = ("ineligible", str(e))
                continue
            ground = _ground_value(prog)
            if ground is not None:
                out[k] = (Assignment(asg.vars, asg.arrays, asg.funcs) if ground else None, prog,
                          0, 0 if ground else -1)
                continue
            keep = distinct(ladder)
            progs.append(prog)
            kept.append(keep)
            free.append([n_free(prog, ladder[r]) for r in keep])
            jobs.append((prog, rows, ladder[keep]))
            where.append(k)
    if not jobs:
        return out
    width = max(1, int(lanes)) if any(any(f) for f in free) else 1
    width = min(width, (1 << 20) // max(len(keep) for keep in kept))   # the call's column cap
    with phase("load"):
        loaded = [(eng.load(p, leafgen(p), prog_seed=0), r, m) for p, r, m in jobs]
    with phase("search"):
        res = eng.carry_ladder(loaded, seed, 0, width)
        for k, (prog, _, masks), f, keep, (first, rung, leaves) in zip(where, jobs, free, kept,
                                                                       res):
            hit = first >= 0
            out[k] = (merge_delta(items[k][1], prog, leaves, masks[rung]) if hit else None, prog,
                      sum(width if x else 1 for x in f), keep[rung] if hit else -1)
    return out


# ---------------------------------------------------------------------------
# Witness sets (MYTHRIL_GPU_CARRY=4): the ladder with several
# pin sets per group, every rung pinning from the rows of its own set
# ---------------------------------------------------------------------------

# pin sets tried per extension (MYTHRIL_GPU_CARRY_SETS, 1..8).  Untuned: 4 is
# enough for the parent and child a JUMPI leaves in the memo and one more pair;
# DESIGN.md §7 round 19 records what sets beyond the first carry
MAX_SETS = 4
SETS_LIMIT = 8                 # include/mythgpu.h MG_CARRY_MAX_SETS


def plan_sets(key: frozenset, memo: HitMemo, max_sets: Optional[int] = None):
    """:func:`plan` with alternatives, a pure function of (key, memo):
    ``("exact", assignment)`` for a remembered key, else ``("extend",
    [(assignment, subset keys taken), ...])`` with at most ``max_sets``
    (default ``MAX_SETS``) pin sets, or None.  Alternative 0 is :func:`plan`'s
    union.  Alternative i > 0 is :func:`union` over ``memo.subsets(key)`` with
    the first subset no earlier alternative took moved to the front, the others
    behind it in their original order — so every remembered subset that
    :func:`union` skipped for a shared name heads a pin set of its own, until
    every subset has been taken by some alternative.  An alternative that
    interprets no name is dropped."""
    hit = memo.hits.get(key)
    if hit is not None:
        return ("exact", hit)
    subs = memo.subsets(key)
    max_sets = MAX_SETS if max_sets is None else max_sets
    alts, covered = [], set()
    for _ in range(max(1, min(int(max_sets), len(subs)))):
        start = next((i for i in range(len(subs)) if i not in covered), None)
        if start is None:
            break
        order = [start] + [i for i in range(len(subs)) if i != start]
        asg, taken = union([memo.hits[subs[i]] for i in order])
        covered.update(order[t] for t in taken)
        if _names(asg):
            alts.append((asg, [subs[order[t]] for t in taken]))
    return ("extend", alts) if alts else None


def sizes_sets(nodes, alts) -> Dict[str, int]:
    """The table sizes of the one program all alternatives of a group are
    evaluated on: per table the maximum of :func:`table_sizes_ck` over the
    alternatives, so every alternative's tables fit."""
    out: Dict[str, int] = {}
    for asg, _ in alts:
        for name, k in table_sizes_ck(nodes, asg).items():
            out[name] = max(out.get(name, 0), k)
    return out


def _mask_bits(mask: np.ndarray, n: int) -> np.ndarray:
    l = np.arange(n)
    return ((mask[l >> 5] >> (l & 31).astype(np.uint32)) & 1).astype(bool)


def rungs_sets(program: Program, alts, nodes):
    """``(rows, masks, rung_set, kept)`` of one job of the ladder with sets:
    ``rows`` ((n_sets, n_leaves, 8) uint32), set s as :func:`rung_masks` gives
    the rows of alternative s of ``alts`` (:func:`plan_sets`'s pairs);
    ``masks`` ((n_rungs, words) uint32) and ``rung_set`` ((n_rungs,) uint32,
    each below n_sets), the rungs in the order they are tried; ``kept``, per
    rung its ``(index in RUNG_NAMES, set)``.  The order is rung-major and
    set-minor — ("all", set 0), ("all", set 1), ..., ("read", set 0), ... — so
    the lowest true column keeps as much of a remembered model as possible and
    alternative 0 wins ties.  A rung whose mask and pinned rows repeat an
    earlier rung's is dropped (rows of leaves the mask leaves free do not
    count); the list is cut at ``MAX_RUNGS``."""
    n = len(program.leaves)
    made = [rung_masks(program, asg, *split_nodes(nodes, taken)) for asg, taken in alts]
    rows = np.stack([r for r, _ in made]).astype(np.uint32).reshape(len(made), n, 8)
    kept, seen = [], set()
    for r in range(len(RUNG_NAMES)):
        for s, (_, ladder) in enumerate(made):
            what = (ladder[r].tobytes(), rows[s][_mask_bits(ladder[r], n)].tobytes())
            if what not in seen:
                seen.add(what)
                kept.append((r, s))
    kept = kept[:MAX_RUNGS]
    masks = np.stack([made[s][1][r] for r, s in kept]).astype(np.uint32)
    return rows, masks, np.array([s for _, s in kept], dtype=np.uint32), kept


def run_sets(eng, items, seed: int, leafgen, lanes: Optional[int] = None, phase=None):
    """:func:`run_ladder` with pin sets: one ``Engine.carry_ladder_sets`` call
    for ``items``, a list of ``(nodes, alts)`` (:func:`plan_sets`'s second
    element).  A group is compiled ONCE, under alternative 0 at the table
    sizes of :func:`sizes_sets`; its alternatives cost columns.  Per item
    ``(assignment, program, candidates, rung, set)`` — as :func:`run_ladder`,
    and the alternative whose rows the hit column pinned (-1 on a miss) — or
    None where the group has no eval form."""
    import contextlib
    from .ir import Unsupported
    phase = phase or (lambda name: contextlib.nullcontext())
    lanes = CARRY_LANES if lanes is None else lanes
    jobs, progs, free, kept, where = [], [], [], [], []
    with phase("compile"):
        for k, (nodes, alts) in enumerate(items):
            try:
                prog = compile_eval_ck(nodes, alts[0][0], sizes_sets(nodes, alts))
                rows, masks, rung_set, keep = rungs_sets(prog, alts, nodes)
            except (Unsupported, ValueError):
                continue
            progs.append(prog)
            kept.append(keep)
            free.append([n_free(prog, m) for m in masks])
            jobs.append((prog, rows, masks, rung_set))
            where.append(k)
    out: List = [None] * len(items)
    if not jobs:
        return out
    width = max(1, int(lanes)) if any(any(f) for f in free) else 1
    width = min(width, (1 << 20) // max(len(keep) for keep in kept))   # the call's column cap
    with phase("load"):
        loaded = [(eng.load(p, leafgen(p), prog_seed=0), r, m, s) for p, r, m, s in jobs]
    with phase("search"):
        res = eng.carry_ladder_sets(loaded, seed, 0, width)
        for k, prog, f, keep, (first, rung, leaves) in zip(where, progs, free, kept, res):
            hit = first >= 0
            out[k] = (unpack(prog, leaves) if hit else None, prog,
                      sum(width if x else 1 for x in f),
                      keep[rung][0] if hit else -1, keep[rung][1] if hit else -1)
    return out


# ---------------------------------------------------------------------------
# The census of a ladder (MYTHRIL_GPU_CARRY=3): which roots
# block on which rung, and the columns a walk starts from
# ---------------------------------------------------------------------------

CARRY_WALKERS = 4              # MYTHRIL_GPU_CARRY_WALKERS: start columns per job
MAX_WALKERS = 64               # include/mythgpu.h MG_CARRY_MAX_WALKERS


def starts_ref(censuses, walkers: int) -> Tuple[np.ndarray, np.ndarray]:
    """The start rule of mg_carry_census (include/mythgpu.h states it), on the
    censuses of a job's rungs over their own columns: ``(start_col,
    start_nfail)``, ``walkers`` entries each.  The list is first the bests of
    the rungs ordered by (failing roots, rung) ascending; then, rung by rung and
    root by root, every ``sole_index`` that is set and is not its rung's best
    column, with 1 failing root.  Start w is list[w]; past the end of the list
    it is list[0] (-1 and 0xFFFFFFFF when no rung counted a column)."""
    cs = list(censuses)
    lst = [(int(c.best_index), int(c.best_nfail))
           for _, c in sorted(enumerate(cs), key=lambda rc: (rc[1].best_nfail, rc[0]))
           if c.best_index >= 0]
    for c in cs:
        for k in range(c.n_roots):
            s = int(c.sole_index[k])
            if s >= 0 and s != c.best_index:
                lst.append((s, 1))
    pad = lst[0] if lst else (-1, 0xFFFFFFFF)
    lst = (lst + [pad] * walkers)[:walkers]
    return (np.array([c for c, _ in lst], dtype=np.int64),
            np.array([f for _, f in lst], dtype=np.uint32))


def compile_census_ck(nodes, asg: Assignment, probes, sizes: Optional[Dict[str, int]] = None
                      ) -> Program:
    """:func:`compile_eval_ck` with caller probes (``census.mask_probes(nodes)``
    first, for a census; the repair's trees add theirs): the same table sizes
    and the same cache, under a key that names the probes."""
    probes = list(probes)
    sizes = table_sizes_ck(nodes, asg) if sizes is None else sizes
    key = ("ck-probes", tuple(n.id for n in nodes), tuple(p.id for p in probes),
           tuple(sorted(sizes.items())))
    prog = _EVAL_CACHE.get(key)
    if prog is not None:
        _EVAL_CACHE.move_to_end(key)
        return prog
    prog = compile_constraints(nodes, probes, solve=False, leaf_pools=True, const_keys=True,
                               table_sizes=sizes or None)
    _EVAL_CACHE[key] = prog
    if len(_EVAL_CACHE) > EVAL_CACHE_SIZE:
        _EVAL_CACHE.popitem(last=False)
    return prog


def run_census(eng, items, seed: int, leafgen, lanes: Optional[int] = None,
               walkers: Optional[int] = None, phase=None):
    """:func:`run_ladder` with a census in place of the gather: one
    ``Engine.carry_census`` call for ``items``, a list of ``(nodes, assignment,
    taken_keys)``.  Per item a dict — ``program`` (the constant-keyed eval form
    with the verdict mask of ``nodes`` as its first probes), ``kept`` (the
    indices in ``RUNG_NAMES`` of the rungs that ran), ``censuses`` (one
    ``census.Census`` per kept rung over that rung's columns), ``start_col``,
    ``start_nfail``, ``starts`` (``Engine.carry_census``), ``lanes``,
    ``assignment`` (start 0 unpacked when it fails no root, else None) and
    ``rung`` (its index in ``RUNG_NAMES``, -1 on a miss) — or None where the
    group has no eval form or more roots than a census takes."""
    import contextlib
    from . import census as CS
    from .ir import Unsupported
    phase = phase or (lambda name: contextlib.nullcontext())
    lanes = CARRY_LANES if lanes is None else lanes
    walkers = CARRY_WALKERS if walkers is None else walkers
    jobs, progs, free, kept, where = [], [], [], [], []
    with phase("compile"):
        for k, (nodes, asg, taken) in enumerate(items):
            if not 1 <= len(nodes) <= CS.MAX_ROOTS:
                continue
            try:
                probes = CS.mask_probes(nodes)
                prog = compile_census_ck(nodes, asg, probes)
                rows, ladder = rung_masks(prog, asg, *split_nodes(nodes, taken))
            except (Unsupported, ValueError):
                continue
            keep = distinct(ladder)
            progs.append(prog)
            kept.append(keep)
            free.append([n_free(prog, ladder[r]) for r in keep])
            jobs.append((CS.census_view(prog, len(probes)), rows, ladder[keep], len(nodes)))
            where.append(k)
    out: List = [None] * len(items)
    if not jobs:
        return out
    width = max(1, int(lanes)) if any(any(f) for f in free) else 1
    width = min(width, (1 << 20) // max(len(keep) for keep in kept))   # the call's column cap
    with phase("load"):
        loaded = [(eng.load(p, leafgen(p), prog_seed=0), r, m, n) for p, r, m, n in jobs]
    with phase("search"):
        res = eng.carry_census(loaded, seed, 0, width, walkers)
        for k, prog, keep, (cs, col, nfail, rows) in zip(where, progs, kept, res):
            hit = int(nfail[0]) == 0
            out[k] = {"program": prog, "kept": keep, "censuses": cs, "start_col": col,
                      "start_nfail": nfail, "starts": rows, "lanes": width,
                      "assignment": unpack(prog, rows[0]) if hit else None,
                      "rung": keep[int(col[0]) // width] if hit else -1}
    return out


def miss_report(nodes, censuses, kept_rungs) -> List[dict]:
    """Why a ladder missed: per kept rung ``{"rung": its name in RUNG_NAMES,
    "n_cand", "best_nfail", "blockers": [{"root": position of the constraint in
    ``nodes``, "constraint": its text, "pass", "first_block", "sole_block"}]}``
    with ``Census.blockers()`` in its order, worst first."""
    nodes = list(nodes)
    out = []
    for r, c in zip(kept_rungs, censuses):
        out.append({"rung": RUNG_NAMES[r], "n_cand": int(c.n_cand),
                    "best_nfail": int(c.best_nfail),
                    "blockers": [{"root": k, "constraint": repr(nodes[k]),
                                  "pass": int(c.pass_[k]),
                                  "first_block": int(c.first_block[k]),
                                  "sole_block": int(c.sole_block[k])} for k in c.blockers()]})
    return out


def run(eng, items, seed: int, leafgen, lanes: Optional[int] = None, phase=None):
    """One ``Engine.carry_batch`` call for ``items``, a list of ``(nodes,
    assignment)``: per item ``(assignment, program, candidates)`` — the witness
    of the group (None on a miss), its eval-form program and the candidates it
    ran — or None where the group has no eval form (``Unsupported``).
    ``leafgen(program)``: the generator parameters of the free leaves
    (``model.search_leafgen``).  A batch none of whose jobs has a free leaf
    runs one candidate; else ``lanes`` (default ``CARRY_LANES``), of which a
    job without a free leaf counts one.  ``phase(name)``: a context manager
    that accounts the compile, load and search steps (``model._Phase``)."""
    import contextlib
    from .ir import Unsupported
    phase = phase or (lambda name: contextlib.nullcontext())
    lanes = CARRY_LANES if lanes is None else lanes
    jobs, progs, free, where = [], [], [], []
    with phase("compile"):
        for k, (nodes, asg) in enumerate(items):
            try:
                prog = compile_eval(nodes, asg)
                mask, rows = pins(prog, asg)
            except (Unsupported, ValueError):
                continue
            progs.append(prog)
            free.append(n_free(prog, mask))
            jobs.append((prog, rows, mask))
            where.append(k)
    out: List = [None] * len(items)
    if not jobs:
        return out
    width = max(1, int(lanes)) if any(free) else 1
    with phase("load"):
        loaded = [(eng.load(p, leafgen(p), prog_seed=0), r, m) for p, r, m in jobs]
    with phase("search"):
        res = eng.carry_batch(loaded, seed, 0, width)
        for k, prog, f, (first, leaves) in zip(where, progs, free, res):
            out[k] = (unpack(prog, leaves) if first >= 0 else None, prog, width if f else 1)
    return out

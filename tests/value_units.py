"""Value parity of bench programs: every node and every root, not their AND.

``tests/test_gpu_bench_parity.py`` compares one bit per lane, the AND of a
unit's ~47 roots, which is almost always 0: a wrong 256-bit value hides
behind any other false conjunct.  This module holds what the value-parity
tests share (``tests/test_value_units.py`` on the CPU with the assembly
simulator as executor, ``tests/test_gpu_value_parity.py`` on the GPU):

* ``UNITS[nreg]``: a fixed list of bench units per register layout, a greedy
  cover of every (family, variant) handler the whole bench configuration
  executes (``engine.handler_variants``) plus a fixed spread;
* three forms of each unit, all compiled as ``bench.compile_unit`` compiles
  (``leaf_remat=bench.BENCH_REMAT``, the layout's ``nreg``, the unit's roots):
  **nodes** (every non-root node of at most 256 bits probed; the roots stay
  constraints, so the ROOT-fused no-write handlers stay), **rootprobe** (every
  root probed inside the full program's register pressure) and **oneroot**
  (one program per root: its bit comes out through its ROOT-fused handler);
* ``check_values``: the one comparison of an executor's results with
  ``oracle/evalref.c``.
"""

import hashlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import bench
from mythril_amd import shard
from mythril_amd.engine import limbs_to_int
from mythril_amd.ir import compile_constraints
from mythril_amd.smt.node import topo_order
from oracle import evalref, gen_ref

SEED = bench.SEED
# 1024 lanes from a nonzero first index: the smallest slice that still spans
# several workgroups
N_LANES, FIRST = 1 << 10, (3 << 20) + 192
WORKLOADS = ("c2", "c3", "c4", "c5")
FORMS = ("nodes", "rootprobe", "oneroot")
# source nodes never probed: constants, and array-sorted terms (a select
# resolves them; they have no value of their own)
SKIP_OPS = ("bvnum", "true", "false", "array", "store", "K")
ORACLE_THREADS = 8

# (workload, unit) per register layout: a greedy cover of the handler
# variants of the whole bench configuration (over the nodes and rootprobe
# programs of every bench unit: most uncovered variants first, ties to the
# shorter program; tests/test_value_units.py asserts it stays a cover), then
# a fixed spread
_SPREAD = ([("c2", d) for d in range(64, 4096, 128)] + [("c3", d) for d in range(0, 256, 32)] +
           [("c4", d) for d in range(0, 256, 32)] + [("c5", d) for d in range(0, 512, 64)])
UNITS = {
    16: [("c3", 205), ("c2", 414), ("c5", 136), ("c2", 3492), ("c3", 149), ("c2", 1696)] + _SPREAD,
    11: [("c2", 996), ("c3", 169), ("c2", 3994), ("c5", 367), ("c2", 3800)] + _SPREAD,
}


def units_of(nreg, workload):
    return [d for w, d in UNITS[nreg] if w == workload]


def _compile(constraints, probes, nreg):
    return compile_constraints(constraints, probes, leaf_remat=bench.BENCH_REMAT, nreg=nreg)


def probe_nodes(roots):
    """(probed, wide): every non-root, non-constant value node of the unit,
    split into those of at most 256 bits (probed) and the wider ones (a probe
    is one 256-bit record; left out, capped by test_left_out_cap)."""
    root_ids = {r.id for r in roots}
    probed, wide = [], []
    for n in topo_order(list(roots)):
        if n.id in root_ids or n.is_array() or n.op in SKIP_OPS:
            continue
        (probed if n.width <= 256 else wide).append(n)
    return probed, wide


class Forms:
    """The bench program of one unit on one layout and its three probed
    forms."""

    def __init__(self, workload, unit, nreg, which=FORMS):
        self.workload, self.unit, self.nreg = workload, unit, nreg
        self.roots = list(bench.workload_roots(workload, unit))
        self.bench = _compile(self.roots, (), nreg)
        self.probes, self.wide = probe_nodes(self.roots)
        names = [(l.name, l.width) for l in self.bench.leaves]
        self.nodes = self.rootprobe = None
        self.oneroot = []
        if "nodes" in which:
            self.nodes = _compile(self.roots, self.probes, nreg)
            assert self.nodes.n_probes == len(self.probes), (workload, unit, nreg)
            assert [(l.name, l.width) for l in self.nodes.leaves] == names, (workload, unit, nreg)
        if "rootprobe" in which:
            self.rootprobe = _compile(self.roots, self.roots, nreg)
            assert self.rootprobe.n_probes == len(self.roots), (workload, unit, nreg)
            assert [(l.name, l.width) for l in self.rootprobe.leaves] == names, (workload, unit)
        if "oneroot" in which:
            self.oneroot = [_compile([r], (), nreg) for r in self.roots]

    def programs(self):
        return [p for p in [self.nodes, self.rootprobe] + self.oneroot if p is not None]


def form_variants(item):
    """Worker: (workload, unit, nreg) -> (bench program's handler variants,
    those of the unit's nodes / rootprobe / oneroot programs)."""
    from mythril_amd.build import LAYOUT_LDS_SLOTS
    from mythril_amd.engine import handler_variants
    w, d, nreg = item
    f = Forms(w, d, nreg)
    lds = LAYOUT_LDS_SLOTS[nreg]
    forms = set()
    for p in f.programs():
        forms |= handler_variants(p, lds)
    return handler_variants(f.bench, lds), forms


# ---------------------------------------------------------------------------
# the oracle's side, computed once per (unit, lane slice) and shared by every
# layout and path (the leaves do not depend on either); units in parallel on
# threads, each oracle call on one
# ---------------------------------------------------------------------------

class Reference:
    """Oracle values of one unit under given leaves: ``values`` (probes, 8,
    n) u32 limbs of every probed node, ``per_root`` (n, roots) bits under the
    same leaves, ``gen_per_root`` the same bits from the oracle's own
    generator."""


_REFS = {}
_ONEROOT = {}


def reference(f, prog, leaves, first, n):
    key = (f.workload, f.unit, first, n)
    ref = _REFS.get(key)
    if ref is not None and np.array_equal(ref.leaves, leaves):
        return ref
    S = evalref.serialize(f.roots, prog, f.probes)
    ref = Reference()
    ref.leaves = leaves.copy()
    _, vals = evalref.run_nodes_soa(S, prog, leaves, [S.node_index[p.id] for p in f.probes])
    # (n, probes, u64 limbs) -> the engine's (probes, 8 u32 limbs, n)
    assert not vals[:, :, 4:].any(), "a probed node wider than 256 bits"
    lo = np.ascontiguousarray(vals[:, :, :4]).view(np.uint32).reshape(n, len(f.probes), 8)
    ref.values = np.ascontiguousarray(lo.transpose(1, 2, 0))
    ref.per_root = evalref.run_leaves_soa(S, prog, leaves, per_root=True, threads=1)
    ref.gen_per_root = evalref.run_gen(S, prog, SEED, f.unit, first, n, 1, per_root=True)
    _REFS[key] = ref
    return ref


def oneroot_reference(f, k, first, n):
    """Root bits of root ``k`` alone, from the oracle's own generator over
    the one-root program's leaves."""
    p = f.oneroot[k]
    dg = hashlib.sha1(repr(([(l.name, l.width) for l in p.leaves],
                            list(p.const_values))).encode()).hexdigest()
    key = (f.workload, f.unit, k, first, n, dg)
    if key not in _ONEROOT:
        _ONEROOT[key] = evalref.run_gen(evalref.serialize([f.roots[k]], p), p, SEED, f.unit,
                                        first, n, 1)
    return _ONEROOT[key]


# ---------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------

def _hex(limbs):
    return "%#x" % limbs_to_int([int(x) for x in limbs])


def _const_table(prog):
    return [sum(int(prog.consts[i, j]) << (32 * j) for j in range(8))
            for i in range(len(prog.const_values))]


def _check_generator(where, f, prog, leaves, first, n):
    table = _const_table(prog)
    for a in sorted({0, 1, n // 2 + 9, n - 1}):
        for li, l in enumerate(prog.leaves):
            want = gen_ref.gen_leaf(SEED, f.unit, li, first + a, l.width, table)
            got = limbs_to_int(leaves[li, :, a])
            assert got == want, "%s unit %d: leaf %d (%s) lane %d: got %#x want %#x" % (
                where, f.unit, li, l.name, a, got, want)


def _check_roots(where, f, bits, ref):
    # the leaves the executor wrote back give what the oracle's own generator
    # gives, root by root; and the launch's root bit is their AND
    bad = np.argwhere(ref.per_root != ref.gen_per_root)
    assert bad.size == 0, "%s unit %d: root %d lane %d: %d under the written-back leaves, %d " \
        "under the oracle's generator" % (where, f.unit, bad[0][1], bad[0][0],
                                          ref.per_root[tuple(bad[0])],
                                          ref.gen_per_root[tuple(bad[0])])
    want = ref.gen_per_root.all(axis=1)
    bad = np.flatnonzero(np.asarray(bits, dtype=bool) != want)
    assert bad.size == 0, "%s unit %d: root bit lane %d: got %d want %d" % (
        where, f.unit, bad[0], bits[bad[0]], want[bad[0]])


def _check_nodes(where, f, probes, ref):
    assert probes.shape == ref.values.shape, (where, f.unit, probes.shape, ref.values.shape)
    is_bool = np.array([p.is_bool() for p in f.probes], dtype=bool)
    diff = probes != ref.values                                    # every limb of a BV
    diff[is_bool] = False
    diff[is_bool, 0, :] = ((probes[is_bool, 0, :] ^ ref.values[is_bool, 0, :]) & 1).astype(bool)
    bad = np.argwhere(diff.any(axis=1))
    if bad.size:
        k, a = (int(x) for x in bad[0])
        p = f.probes[k]
        raise AssertionError(
            "%s unit %d: node %d (%s, %s %d bits) lane %d: got %s want %s (%d node values differ)"
            % (where, f.unit, k, p.op, "Bool" if p.is_bool() else "BV", p.width, a,
               _hex(probes[k, :, a]), _hex(ref.values[k, :, a]), len(bad)))


def check_values(executor, workload, nreg, path, units, first=FIRST, n=N_LANES, forms=FORMS):
    """Run the ``forms`` of ``units`` (bench units of ``workload``, compiled
    for ``nreg`` slots) through ``executor`` and compare with the oracle.

    ``executor.session(items)``: a context manager entered once with every
    ``(unit, program)`` item of the call (a GPU executor loads them and
    attaches one compiled image).
    ``executor.probed(items, first, n)``: per ``(unit, program)`` item the
    ``(root bits, probes, leaves)`` of ``Engine.eval_gen(..., want_probes=True,
    want_leaves=True)`` (generator seed ``SEED``, ``prog_seed`` = unit).
    ``executor.batch(items, first, n)``: ``(bits (items, n) bool, first
    satisfying indices or None)`` of all items in one ``batch_eval_gen``.

    Checked: every probed node's value (all 8 limbs of a BV, so the limbs
    above its width are zero; bit 0 of a Bool) under the leaves the executor
    wrote back; the launch's root bit against ``evalref.run_gen`` on every
    lane; the written-back leaves against ``oracle/gen_ref.py`` on sampled
    lanes; every root's probe bit (rootprobe); every one-root program's bits
    and first satisfying index (oneroot).  Raises AssertionError naming
    workload, layout, path, unit, node, lane, got and want.  Returns
    ``{"units", "nodes", "roots", "mixed"}``: units run, node values compared
    per lane, roots compared, and roots whose bit is true on some lanes of
    the slice and false on others."""
    fs = [Forms(workload, d, nreg, forms) for d in units]
    with executor.session([(f.unit, p) for f in fs for p in f.programs()]):
        return _check_forms(executor, fs, "%s %d-slot %s" % (workload, nreg, path), first, n, forms)


def _check_forms(executor, fs, where, first, n, forms):
    stats = {"units": len(fs), "nodes": 0, "roots": 0, "mixed": 0}

    def refs(tag, progs, res):
        with ThreadPoolExecutor(max_workers=ORACLE_THREADS) as ex:    # ctypes drops the GIL
            out = list(ex.map(lambda t: reference(t[0], t[1], t[2][2], first, n),
                              zip(fs, progs, res)))
        for f, p, (_, _, leaves) in zip(fs, progs, res):
            _check_generator("%s %s" % (where, tag), f, p, leaves, first, n)
        return out

    if "nodes" in forms:
        progs = [f.nodes for f in fs]
        res = executor.probed([(f.unit, f.nodes) for f in fs], first, n)
        for f, (bits, probes, _), ref in zip(fs, res, refs("nodes", progs, res)):
            _check_roots(where + " nodes", f, bits, ref)
            _check_nodes(where + " nodes", f, probes, ref)
            stats["nodes"] += len(f.probes)
    if "rootprobe" in forms:
        progs = [f.rootprobe for f in fs]
        res = executor.probed([(f.unit, f.rootprobe) for f in fs], first, n)
        for f, (bits, probes, _), ref in zip(fs, res, refs("rootprobe", progs, res)):
            _check_roots(where + " rootprobe", f, bits, ref)
            got = (probes[:, 0, :] & 1).astype(bool).T                   # (n, roots)
            bad = np.argwhere(got != ref.per_root)
            if bad.size:
                a, k = (int(x) for x in bad[0])
                raise AssertionError(
                    "%s rootprobe unit %d: root %d (%s) lane %d: got %s want %d"
                    % (where, f.unit, k, f.roots[k].op, a, _hex(probes[k, :, a]),
                       ref.per_root[a, k]))
            stats["roots"] += len(f.roots)
            col = ref.gen_per_root
            stats["mixed"] += int((col.any(axis=0) & ~col.all(axis=0)).sum())
    if "oneroot" in forms:
        items = [(f.unit, p) for f in fs for p in f.oneroot]
        bits, firsts = executor.batch(items, first, n)
        i = 0
        for f in fs:
            for k in range(len(f.roots)):
                want = oneroot_reference(f, k, first, n)
                bad = np.flatnonzero(np.asarray(bits[i], dtype=bool) != want)
                assert bad.size == 0, "%s oneroot unit %d: root %d (%s) lane %d: got %d want %d" % (
                    where, f.unit, k, f.roots[k].op, bad[0], bits[i][bad[0]], want[bad[0]])
                if firsts is not None:
                    hit = np.flatnonzero(want)
                    idx = first + int(hit[0]) if hit.size else shard.NONE
                    assert firsts[i] == idx, "%s oneroot unit %d: root %d (%s): first " \
                        "satisfying index %#x, want %#x" % (where, f.unit, k, f.roots[k].op,
                                                            firsts[i], idx)
                if "rootprobe" not in forms:
                    stats["roots"] += 1
                    stats["mixed"] += int(want.any() and not want.all())
                i += 1
    return stats


def informative_roots(workload, unit, first=FIRST, n=N_LANES):
    """(roots with mixed true / false lanes, roots) of a bench unit on the
    slice, by the oracle alone (its own generator on the bench program)."""
    roots = list(bench.workload_roots(workload, unit))
    prog = _compile(roots, (), 16)
    col = evalref.run_gen(evalref.serialize(roots, prog), prog, SEED, unit, first, n,
                          ORACLE_THREADS, per_root=True)
    return int((col.any(axis=0) & ~col.all(axis=0)).sum()), len(roots)

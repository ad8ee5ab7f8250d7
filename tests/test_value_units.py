"""CPU side of the value-parity tests (tests/value_units.py; the GPU side is
tests/test_gpu_value_parity.py).

* the oracle helper that returns node values is pinned to
  ``oracle/smtlib_ref.py``;
* ``UNITS[nreg]`` covers every (family, variant) handler the whole bench
  configuration executes, leaves out few nodes, and has informative roots;
* ``check_values`` notices one corrupted limb of one spill / reload handler
  that the root-AND bit (all that test_gpu_bench_parity.py compares) does
  not (the assembly simulator as executor).

Measured on the slice (1024 lanes from ``FIRST``, oracle alone), roots with
both true and false lanes over ``UNITS``:

    layout  C2                 C3               C4               C5
    16      1255 / 1603 (78 %) 232 / 475 (49 %) 127 / 245 (52 %) 102 / 189 (54 %)
    11      1261 / 1602 (79 %) 201 / 405 (50 %) 127 / 245 (52 %)  94 / 173 (54 %)

and non-root, non-constant nodes left unprobed for being wider than 256
bits: C2 0; C3 1.5 % / 1.6 %; C4 2.0 %; C5 2.4 % / 2.0 % (16 / 11 slots).
"""

import contextlib
import os

import numpy as np
import pytest

import asm_sim
import bench
import value_units as V
from mythril_amd import asmgen
from mythril_amd.assign import unpack
from mythril_amd.build import LAYOUT_LDS_SLOTS
from mythril_amd.engine import default_leafgen, handler_variants, record_handlers
from mythril_amd.procmap import process_map
from oracle import evalref, gen_ref
from oracle import smtlib_ref as R

WORKERS = min(16, os.cpu_count() or 1)


@pytest.mark.parametrize("workload,unit", [("c2", 5), ("c4", 3)])
def test_oracle_node_values_match_python_oracle(workload, unit):
    """``evalref.run_nodes_soa`` (every node's value under an engine-shaped
    leaf buffer, lanes in chunks) and ``run_gen(per_root=True)`` against
    ``smtlib_ref.evaluate`` on a few generated lanes of a bench unit."""
    f = V.Forms(workload, unit, 16, ("nodes",))
    prog, lanes, first = f.nodes, 5, V.FIRST + 40
    pool = prog.const_values
    leaves = np.zeros((len(prog.leaves), 8, lanes), dtype=np.uint32)
    for a in range(lanes):
        for li, l in enumerate(prog.leaves):
            v = gen_ref.gen_leaf(V.SEED, unit, li, first + a, l.width, pool)
            leaves[li, :, a] = [(v >> (32 * j)) & 0xFFFFFFFF for j in range(8)]
    S = evalref.serialize(f.roots, prog, f.probes)
    nodes = f.probes + f.wide + f.roots
    recs = [S.node_index[p.id] for p in nodes]
    bits, every = evalref.run_nodes_soa(S, prog, leaves, chunk=2)            # 2 + 2 + 1 lanes
    _, some = evalref.run_nodes_soa(S, prog, leaves, recs)
    assert every.shape[:2] == (lanes, len(S.recs)) and some.shape[:2] == (lanes, len(nodes))
    assert np.array_equal(every[:, recs, :], some)
    per_root = evalref.run_gen(S, prog, V.SEED, unit, first, lanes, 1, per_root=True)
    for a in range(lanes):
        asg = unpack(prog, leaves[:, :, a])
        want = R.evaluate(nodes, R.Assignment(asg.vars, asg.arrays, asg.funcs))
        got = [evalref.node_value(some, a, k) for k in range(len(nodes))]
        assert got == [int(w) for w in want], (workload, unit, a)
        assert [int(b) for b in per_root[a]] == [int(w) for w in want[-len(f.roots):]]
        assert bool(bits[a]) == all(want[-len(f.roots):])


def _bench_variants(item):
    w, d, nreg = item
    return handler_variants(bench.compile_unit((w, d, nreg))[1], LAYOUT_LDS_SLOTS[nreg])


@pytest.mark.parametrize("nreg", [16, 11])
def test_units_cover_every_bench_handler_variant(nreg):
    """Every (family, variant) handler that a program of the whole bench
    configuration executes on this layout is executed by a nodes, rootprobe
    or oneroot program of ``UNITS[nreg]``.  A missing variant means: extend
    ``UNITS``."""
    items = [(w, d, nreg) for w in V.WORKLOADS for d in range(bench.default_units(w))]
    bench_set = set().union(*process_map(_bench_variants, items, WORKERS, "spawn", chunksize=64))
    covered = set()
    for hb, hf in process_map(V.form_variants, [(w, d, nreg) for w, d in V.UNITS[nreg]],
                              WORKERS, "spawn", chunksize=2):
        covered |= hf
    print("%d-slot layout: the bench configuration executes %d (family, variant) handlers, the "
          "probed programs of %d units %d" % (nreg, len(bench_set), len(V.UNITS[nreg]),
                                              len(covered)))
    assert sorted(bench_set - covered) == []
    for w in V.WORKLOADS:
        assert len(V.units_of(nreg, w)) >= (32 if w == "c2" else 8), w
    assert len(set(V.UNITS[nreg])) == len(V.UNITS[nreg])


@pytest.mark.parametrize("nreg", [16, 11])
def test_left_out_cap(nreg):
    """Nodes wider than 256 bits cannot be probed; they are none of C2's and
    at most 3 % of each stream's non-root, non-constant nodes over UNITS."""
    for w in V.WORKLOADS:
        probed = wide = 0
        for d in V.units_of(nreg, w):
            p, x = V.probe_nodes(bench.workload_roots(w, d))
            probed, wide = probed + len(p), wide + len(x)
        print("%s %d-slot: %d nodes probed, %d left out (%.2f %%)"
              % (w, nreg, probed, wide, 100.0 * wide / (probed + wide)))
        assert wide == 0 if w == "c2" else wide <= 0.03 * (probed + wide), (w, probed, wide)


@pytest.mark.parametrize("nreg", [16, 11])
def test_roots_are_informative(nreg):
    """By the oracle alone, on the slice the value tests run: at least half
    of C2's roots and a quarter of each stream's are true on some lanes and
    false on others (a root constant on the slice checks one value)."""
    for w in V.WORKLOADS:
        mixed = roots = 0
        for d in V.units_of(nreg, w):
            m, r = V.informative_roots(w, d)
            mixed, roots = mixed + m, roots + r
        print("%s %d-slot: %d of %d roots mixed (%.1f %%)" % (w, nreg, mixed, roots,
                                                              100.0 * mixed / roots))
        assert mixed >= (0.5 if w == "c2" else 0.25) * roots, (w, mixed, roots)


class SimExecutor:
    """One 64-lane wave of the generated interpreter text (16-slot layout)."""

    def session(self, items):
        return contextlib.nullcontext()

    def probed(self, items, first, n):
        assert n == asm_sim.NL
        out = []
        for unit, prog in items:
            root, probes, leaves, _ = asm_sim.simulate(
                prog, gen=(V.SEED, unit, first, default_leafgen(prog)), n_lds=LAYOUT_LDS_SLOTS[16],
                want_leaves=True)
            out.append((root, probes[:prog.n_probes], leaves[:len(prog.leaves)]))
        return out

    def batch(self, items, first, n):
        return np.array([self.probed([it], first, n)[0][0] for it in items]), None


# the corrupted handler: the full-width LDS reload into a slot; its second
# ds_read_b128 (limbs 4..7) is made to fill limbs 4..7 from the region's first
# half, so limb 4 (and 5..7) of every value reloaded into that slot is wrong
SENSITIVITY_UNIT = ("c2", 1696)


def _executed_labels(prog, family):
    """(label id, variant) of the ``family`` handlers ``prog`` executes."""
    out = []
    with asmgen.layout(prog.nreg):
        for h in record_handlers(prog, LAYOUT_LDS_SLOTS[prog.nreg]):
            c = asmgen.canonical(h)
            if asmgen.AOPS[c // (2 * asmgen.NVAR)] == family and (c, (c // 2) % asmgen.NVAR) not in out:
                out.append((c, (c // 2) % asmgen.NVAR))
    return out


def test_check_values_sees_a_corrupted_reload_the_root_bit_does_not():
    """``check_values`` passes on the generated interpreter (nodes and
    rootprobe forms of a UNITS program that spills, one simulated wave), and
    fails when one instruction of a RELOAD_LDS handler the program executes
    is edited: the full-width variant's second ``ds_read_b128`` (the
    handler has no narrower access to edit) then fills limbs 4..7 from the
    region's low half.  Under the same edit the root bit of the nodes
    program and of the unit's bench program itself, which executes the same
    handler, is unchanged on all 64 lanes: what test_gpu_bench_parity.py
    compares cannot see it.  (Every RELOAD_LDS slot variant both programs
    execute is tried; one whose edit changes no probed value at all is
    passed over, at least one must change some.)"""
    w, d = SENSITIVITY_UNIT
    assert asmgen.NREG == 16 and (w, d) in V.UNITS[16]
    first, n, ex = V.FIRST, asm_sim.NL, SimExecutor()
    f = V.Forms(w, d, 16, ("nodes",))
    clean = ex.probed([(d, f.nodes), (d, f.bench)], first, n)
    stats = V.check_values(ex, w, 16, "sim", [d], first, n, forms=("nodes", "rootprobe"))
    assert stats["nodes"] == len(f.probes) and stats["roots"] == len(f.roots)
    # a full-width RELOAD_LDS that both the nodes program and the bench
    # program of the unit execute
    both = [x for x in _executed_labels(f.nodes, "RELOAD_LDS")
            if x in _executed_labels(f.bench, "RELOAD_LDS") and not x[1] & asmgen.V_NARROW]
    assert both
    lines, _ = asm_sim.body_and_table()
    saved = list(lines)
    try:
        seen = 0
        for label, _ in both:
            at = next(i for i, t in enumerate(saved) if t.strip().startswith(".Lh%d_" % label))
            reads = [i for i in range(at + 1, at + 40) if "ds_read_b128" in saved[i]][:2]
            lo, hi = saved[reads[0]].split(","), saved[reads[1]].split(",")
            corrupted = list(saved)
            corrupted[reads[1]] = ",".join(hi[:1] + lo[1:])       # limbs 4..7 <- the low half
            assert corrupted[reads[1]] != saved[reads[1]]
            asm_sim._CACHE["lines"] = corrupted
            bad = ex.probed([(d, f.nodes), (d, f.bench)], first, n)
            # the blindness: the root-AND bit of both programs is what it was
            assert np.array_equal(bad[0][0], clean[0][0]) and np.array_equal(bad[1][0], clean[1][0])
            if np.array_equal(bad[0][1], clean[0][1]):
                continue          # every value reloaded into this slot is short, or read low
            with pytest.raises(AssertionError, match=r"c2 16-slot sim nodes unit 1696: node \d+ "):
                V.check_values(ex, w, 16, "sim", [d], first, n, forms=("nodes",))
            seen += 1
        assert seen, "no edit changed a node value: pick another handler"
    finally:
        asm_sim._CACHE["lines"] = saved
    V.check_values(ex, w, 16, "sim", [d], first, n, forms=("nodes",))


def test_batch_comparison_rejects_a_wrong_lane_and_a_wrong_first_index():
    """``gpu_batch.assert_matches_oracle`` (the one root-bit comparison of the
    GPU parity tests) passes on the oracle's own data and fails on one
    flipped lane, a first index off by one, and ``shard.NONE`` where a hit
    exists: 3 units x 128 made-up lanes, the middle one with no hit."""
    import gpu_batch as G
    from mythril_amd import shard
    first = 1 << 20
    want = np.zeros((3, 128), dtype=bool)
    want[0, [70, 127]] = want[2, 5] = True
    firsts = [first + 70, shard.NONE, first + 5]
    assert G.assert_matches_oracle(want.copy(), firsts, want, first, "made up") == (2, 3)
    for unit, lane in ((0, 3), (1, 64), (2, 5)):
        bad = want.copy()
        bad[unit, lane] ^= True
        with pytest.raises(AssertionError, match=r"'made up', %d, %d\)" % (unit, lane)):
            G.assert_matches_oracle(bad, firsts, want, first, "made up")
    for unit, idx in ((0, first + 71), (0, first + 69), (2, shard.NONE), (1, first)):
        wrong = list(firsts)
        wrong[unit] = idx
        with pytest.raises(AssertionError, match=r"'made up', %d\)" % unit):
            G.assert_matches_oracle(want, wrong, want, first, "made up")

"""The delta carry on the host (MYTHRIL_GPU_CARRY=5): the two
masks of carry.delta_job, its refusal, carry.merge_delta, and the whole flow
without a device — carry.run_delta on an engine whose ``carry_ladder`` is the
host lane function (mg_carry_fill_rungs_host) under oracle/evalref — on a trap,
on ground programs, through model._carry_groups, and over stream replays.  A
hit is never judged on the delta program alone: EVERY node of the whole group
is evaluated under the merged assignment by oracle/smtlib_ref.  CPU only."""

import numpy as np
import pytest

import mythril_amd.model as M
from mythril_amd import carry as CY
from mythril_amd import engine as E
from mythril_amd import workloads as W
from mythril_amd.assign import Assignment, lookup, unpack
from mythril_amd.ir import Unsupported, compile_constraints
from mythril_amd.smt import node as N
from delta_cases import (SEED, CpuEngine, by_leaf, byte, calldata_group, holds, key_of, run_delta,
                         trap, witness)
from oracle import evalref


# ---------------------------------------------------------------------------
# a crafted parent and child (delta_cases.calldata_group)
# ---------------------------------------------------------------------------

def test_all_is_pins_and_read_strict_frees_the_cval_leaf_the_parent_never_read():
    parent, new = calldata_group()
    asg = witness()
    assert holds(parent, asg) == [] and holds(new, asg) == [0]
    prog, rows, ladder = CY.delta_job(parent + new, asg, [key_of(parent)])
    # the new node alone, with constant keys, from the ladder's cache
    assert prog is CY.compile_eval_ck(new, asg, CY.table_sizes_ck(new, asg))
    assert prog.table_ckeys["dcd"] == [4] and [l.kind for l in prog.leaves] == ["cval"]
    assert len(prog.code) < len(CY.compile_eval_ck(parent + new, asg).code)
    mask, prows = CY.pins(prog, asg)
    assert ladder.shape == (2, 1) and ladder.dtype == np.uint32
    assert np.array_equal(ladder[0], mask) and np.array_equal(rows, prows)
    assert by_leaf(prog, ladder[0]) == {("cval", "dcd", 0)} and by_leaf(prog, ladder[1]) == set()
    # a key the parent did read stays pinned on both rungs
    again = [N.bv_cmp("bvugt", byte(N.array_var("dcd", 256, 8), 3), N.bv_num(5, 8))]
    prog, rows, ladder = CY.delta_job(parent + again, asg, [key_of(parent)])
    assert prog.table_ckeys["dcd"] == [3] and np.array_equal(ladder[0], ladder[1])
    assert CY.distinct(ladder) == [0] and CY.n_free(prog, ladder[0]) == 0


def test_read_strict_frees_nothing_of_a_table_the_parent_reads_at_a_symbolic_key():
    parent, new = calldata_group(sym_read=True)
    asg = witness()
    assert holds(parent, asg) == []
    prog, rows, ladder = CY.delta_job(parent + new, asg, [key_of(parent)])
    assert by_leaf(prog, ladder[0]) == by_leaf(prog, ladder[1]) == {("cval", "dcd", 0)}
    assert CY.distinct(ladder) == [0]
    # the ladder's "read" DOES free that leaf (it evaluates the parent's roots again): the
    # scan lists the table, 4 numeral keys x 1 symbolic read
    lax = CY.rung_masks(prog, asg, parent, new)[1]
    assert by_leaf(prog, lax[0]) == {("cval", "dcd", 0)} and by_leaf(prog, lax[1]) == set()
    # a key list the scan had to cut frees nothing either
    from mythril_amd import ir
    cd = N.array_var("dcd", 256, 8)
    wide = [N.bv_cmp("bvule", byte(cd, 1000 + k), N.bv_num(255, 8)) for k in range(ir.CKEY_CAP)]
    assert len(ir.scan_const_keys(wide + [N.eq(byte(cd, 7), N.bv_num(0, 8))])["dcd"]) == ir.CKEY_CAP
    prog, rows, ladder = CY.delta_job(wide + new, asg, [key_of(wide)])
    assert np.array_equal(ladder[0], ladder[1])


def test_a_parent_symbol_the_witness_does_not_interpret_is_refused():
    parent, new = calldata_group()
    w = N.bv_var("dw", 256)
    parent = parent + [N.bv_cmp("bvult", w, N.bv_num(7, 256))]
    child = new + [N.bv_cmp("bvugt", w, N.bv_num(2, 256))]
    with pytest.raises(ValueError, match="silent about dw"):
        CY.delta_job(parent + child, witness(), [key_of(parent)])      # the witness lacks dw
    asg = witness()
    asg.vars["dw"] = 1
    prog, rows, ladder = CY.delta_job(parent + child, asg, [key_of(parent)])
    assert ("var", "dw", 0) in by_leaf(prog, ladder[1])
    # a symbol of the new nodes alone is fresh, not a refusal
    u = N.bv_var("du", 256)
    prog, rows, ladder = CY.delta_job(parent + new + [N.bv_cmp("bvugt", u, w)], asg,
                                      [key_of(parent)])
    assert ("var", "du", 0) not in by_leaf(prog, ladder[0])
    # the same for a table, and for a group with nothing new
    f = N.apply_uf("df", 256, 256, w)
    p2 = parent + [N.eq(N.bv_op("bvand", f, N.bv_num(0, 256)), N.bv_num(0, 256))]
    with pytest.raises(ValueError, match="silent about df"):
        CY.delta_job(p2 + [N.bv_cmp("bvugt", f, N.bv_num(2, 256))], asg, [key_of(p2)])
    with pytest.raises(ValueError, match="no delta"):
        CY.delta_job(parent, asg, [key_of(parent)])
    res = run_delta([(parent + child, witness(), [key_of(parent)])])
    assert res[0][0] == "ineligible" and "dw" in res[0][1]


def test_merge_writes_the_freed_key_and_the_fresh_symbols_and_nothing_else():
    parent, new = calldata_group()
    u = N.bv_var("du", 256)
    g = N.apply_uf("dg", 256, 256, u)
    new = new + [N.bv_cmp("bvugt", u, N.bv_num(9, 256)), N.eq(g, N.bv_num(5, 256))]
    asg = Assignment(vars={"dv": 1, "dz": 9},
                     arrays={"dcd": ([(k, 0xA0 + k) for k in range(4)], 0x33)},
                     funcs={"dh": ([(1, 2)], 3)})
    before = repr(asg)
    prog, rows, ladder = CY.delta_job(parent + new, asg, [key_of(parent)])
    leaves = rows.copy()
    for l, leaf in enumerate(prog.leaves):
        if leaf.kind == "cval" and leaf.source == "dcd":
            leaves[l, 0] = 0x77
        elif leaf.source == "du":
            leaves[l, 0] = 10
        elif leaf.source == "dg":                             # every key 10, every value 5
            leaves[l, 0] = {"key": 10, "val": 5}.get(leaf.kind, 0)
    # rung "read": byte 4 is ADDED to the carried table, the fresh var and function come in whole
    m = CY.merge_delta(asg, prog, leaves, ladder[1])
    assert repr(asg) == before                                # a copy: the memo's witness is intact
    assert m.arrays["dcd"][1] == 0x33 and sorted(m.arrays["dcd"][0]) == \
        [(0, 0xA0), (1, 0xA1), (2, 0xA2), (3, 0xA3), (4, 0x77)]
    assert m.vars == {"dv": 1, "dz": 9, "du": 10} and m.funcs["dh"] == ([(1, 2)], 3)
    assert lookup(m.funcs["dg"], 10) == 5 and set(m.funcs) == {"dh", "dg"}
    assert holds(parent + new, m) == []
    # rung "all": the same column changes no carried table at all
    m0 = CY.merge_delta(asg, prog, leaves, ladder[0])
    assert m0.arrays == asg.arrays and m0.vars == m.vars and m0.funcs == m.funcs
    # a don't-care entry at the freed key is overwritten, wherever it stands, and no other
    asg.arrays["dcd"] = ([(4, 0xA4)] + [(k, 0xA0 + k) for k in range(4)] + [(9, 1), (4, 0xEE)],
                         0x33)
    prog, rows, ladder = CY.delta_job(parent + new, asg, [key_of(parent)])
    m = CY.merge_delta(asg, prog, leaves, ladder[1])
    assert lookup(m.arrays["dcd"], 4) == 0x77 and 0xA4 not in dict(m.arrays["dcd"][0]).values()
    assert sorted(m.arrays["dcd"][0]) == \
        [(0, 0xA0), (1, 0xA1), (2, 0xA2), (3, 0xA3), (4, 0x77), (9, 1)]
    assert holds(parent + new, m) == []


# ---------------------------------------------------------------------------
# the flow: a hit, the trap, ground programs
# ---------------------------------------------------------------------------

def test_the_child_hits_on_read_strict_and_the_whole_group_holds():
    parent, new = calldata_group()
    eng = CpuEngine()
    (r,) = run_delta([(parent + new, witness(), [key_of(parent)])], eng)
    asg, prog, cand, rung = r
    assert rung == 1 and cand == 1 + CY.CARRY_LANES and eng.calls == 1
    assert lookup(asg.arrays["dcd"], 4) == 0x77 and len(prog.leaves) == 1
    assert holds(parent + new, asg) == []
    # under a symbolic read of the parent it misses: one rung, one candidate
    parent, new = calldata_group(sym_read=True)
    (r,) = run_delta([(parent + new, witness(), [key_of(parent)])])
    assert r[0] is None and r[2:] == (1, -1)


def test_the_trap_misses_on_both_rungs_and_the_lax_mask_would_have_broken_the_parent():
    parent, new, asg = trap()
    assert holds(parent, asg) == [] and holds(new, asg) == [0]
    prog, rows, ladder = CY.delta_job(parent + new, asg, [key_of(parent)])
    assert by_leaf(prog, ladder[0]) == by_leaf(prog, ladder[1]) == {("cval", "dtrap", 0)}
    (r,) = run_delta([(parent + new, asg, [key_of(parent)])])
    assert r[0] is None and r[3] == -1
    # each rung on its own, on the oracle's columns: nothing
    for m in ladder:
        soa = E.carry_fill_rungs_host(M.search_leafgen(prog), prog.consts, 0, rows, m[None, :],
                                      SEED, 0, CY.CARRY_LANES)
        assert not evalref.run_leaves_soa(evalref.serialize(new, prog), prog, soa).any()
    # the ladder's "read" frees T[5]: the delta program is satisfied by T[5] = 2 ...
    lax = CY.rung_masks(prog, asg, parent, new)[1][1]
    assert by_leaf(prog, lax) == set()
    col = rows.copy()
    col[0] = 0
    col[0, 0] = 2
    assert evalref.run_leaves_soa(evalref.serialize(new, prog), prog,
                                  np.ascontiguousarray(col[:, :, None])).tolist() == [True]
    # ... and the merged assignment fails the parent's first root: select(T, x) is now 2
    bad = CY.merge_delta(asg, prog, col, lax)
    assert lookup(bad.arrays["dtrap"], 5) == 2 and holds(parent + new, bad) == [0]


def test_a_ground_delta_is_answered_without_a_launch():
    parent, _ = calldata_group()
    v = N.bv_var("dv", 256)
    zero = N.bv_num(0, 256)
    folds = N.bool_val(True)
    never = N.eq(N.bv_op("bvmul", v, zero), N.bv_num(1, 256))    # false whatever dv is
    eng = CpuEngine()
    asg = witness()
    yes, no = run_delta([(parent + [folds], asg, [key_of(parent)]),
                         (parent + [never], asg, [key_of(parent)])], eng)
    assert eng.calls == 0
    assert M._ground_value(yes[1]) is True and M._ground_value(no[1]) is False
    assert yes[2:] == (0, 0) and repr(yes[0]) == repr(asg) and yes[0] is not asg
    assert holds(parent + [folds], yes[0]) == []
    assert no[0] is None and no[2:] == (0, -1)
    # a fold that keeps its leaf (the leaf table is the plain lowering's) is not ground: one
    # pinned candidate, a hit on "all"; so is a program of numerals alone, with no leaf at all
    kept = N.eq(N.bv_op("bvand", v, zero), zero)
    plain = N.eq(N.bv_op("bvadd", N.bv_num(1, 256), N.bv_num(1, 256)), N.bv_num(2, 256))
    a, b = run_delta([(parent + [kept], asg, [key_of(parent)]),
                      (parent + [plain], asg, [key_of(parent)])], eng)
    assert eng.calls == 1 and M._ground_value(a[1]) is None and M._ground_value(b[1]) is None
    assert a[2:] == (1, 0) and b[2:] == (1, 0) and len(a[1].leaves) == 1 and not b[1].leaves
    assert repr(a[0]) == repr(asg) == repr(b[0])


# ---------------------------------------------------------------------------
# the knob, the counters, model._carry_groups
# ---------------------------------------------------------------------------

def test_knob_5_selects_the_delta_and_its_counters_print_only_when_there_are():
    try:
        M.configure_from_env({"MYTHRIL_GPU_CARRY": "5"})
        assert M.CARRY == "delta"
        for value, want in (("4", "sets"), ("2", "ladder"), ("1", True), ("0", False)):
            M.configure_from_env({"MYTHRIL_GPU_CARRY": value})
            assert M.CARRY == want
    finally:
        M.configure_from_env()
    assert M.CARRY is False
    s = M.SolverStatistics()
    s.carry_attempts, s.carry_hits, s.carry_candidates = 2, 1, 513
    assert repr(s).endswith("GPU carry: exact: 0 attempts: 2 hits: 1 candidates: 513")
    s.carry_delta_attempts, s.carry_delta_hits = 2, [0, 1]
    s.carry_delta_roots, s.carry_delta_group_roots = 2, 12
    assert repr(s).endswith("candidates: 513 delta attempts: 2 delta hits: 0/1 ineligible: 0 "
                            "roots: 2 of 12")
    s.reset_gpu()
    assert (s.carry_delta_attempts, s.carry_delta_hits, s.carry_delta_ineligible,
            s.carry_delta_roots) == (0, [0, 0], 0, 0)


def test_carry_groups_notes_a_delta_hit_and_hands_the_refused_group_to_the_ladder(monkeypatch):
    parent, new = calldata_group()
    w = N.bv_var("dw", 256)
    p2 = [N.bv_cmp("bvult", w, N.bv_num(7, 256)),
          N.eq(N.bv_op("bvand", N.bv_var("dq", 256), N.bv_num(0, 256)), N.bv_num(0, 256))]
    c2 = p2 + [N.bv_cmp("bvugt", N.bv_var("dq", 256), N.bv_num(2, 256))]
    tp, tn, tasg = trap()
    M.clear_search_memos()
    M.stats.reset_gpu()
    s = M.stats
    try:
        monkeypatch.setattr(M, "CARRY", "delta")
        M._note_hit(key_of(parent), witness(68))                # 68 entries, read at constants
        M._note_hit(key_of(p2), Assignment(vars={"dw": 1}))     # silent about dq: it folded away
        M._note_hit(key_of(tp), tasg)
        groups = [(key_of(g), g) for g in (parent + new, c2, tp + tn)]
        eng = CpuEngine()
        eng.know([(parent + new, witness(68), [key_of(parent)]), (tp + tn, tasg, [key_of(tp)])])
        seen = []

        def ladder(e, items, seed, leafgen, lanes=None, phase=None):
            seen.extend(items)
            return [None] * len(items)
        monkeypatch.setattr(CY, "run_ladder", ladder)
        out = M._carry_groups(groups, eng=eng)
        assert list(out) == [key_of(parent + new)] and eng.calls == 1
        asg, prog = out[key_of(parent + new)]
        assert holds(parent + new, asg) == [] and len(asg.arrays["dcd"][0]) == 68
        assert M._hit_memo.hits[key_of(parent + new)] is asg
        assert len(prog.code) < len(CY.compile_eval_ck(parent + new, witness(68)).code)
        assert (s.carry_delta_attempts, s.carry_delta_hits, s.carry_delta_ineligible) == \
            (2, [0, 1], 1)
        assert (s.carry_delta_roots, s.carry_delta_group_roots) == (2, 9)   # 1 of 6, 1 of 3
        assert (s.carry_attempts, s.carry_hits, s.carry_gated) == (2, 1, 0)
        assert s.carry_rung_hits == [0, 0, 0]                   # the ladder's own: untouched
        assert (s.kernel_calls, s.launches) == (1, 3)
        # the refused group went to the ladder in the same call, the trap's miss did not
        assert [key_of(i[0]) for i in seen] == [key_of(c2)] and seen[0][2] == [key_of(p2)]
        assert "delta attempts: 2 delta hits: 0/1 ineligible: 1 roots: 2 of 9" in repr(s)
        # the table gate looks at the NEW nodes' tables
        ps, ns = calldata_group(sym_read=True)
        extra = ns + [N.eq(N.select(N.array_var("dcd", 256, 8),
                                    N.bv_op("bvadd", N.bv_var("dv", 256), N.bv_num(1, 256))),
                           N.bv_num(0xA2, 8))]
        assert CY.table_sizes_ck(extra, witness(68)) == {"dcd": 67}
        M._note_hit(key_of(ps), witness(68))
        assert M._carry_groups([(key_of(ps + extra), ps + extra)], eng=eng) == {}
        assert s.carry_gated == 1 and s.carry_delta_attempts == 2
    finally:
        M.clear_search_memos()
        M.stats.reset_gpu()


# ---------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------

SEARCH = 4096                                  # candidates of the stand-in search below


def cpu_search(nodes):
    """A witness of ``nodes`` among the generator's first ``SEARCH`` candidates
    of the eval form, found by the oracle, or None: what fills the memo here
    in place of the device search."""
    try:
        prog = compile_constraints(nodes, solve=False, leaf_pools=True, const_keys=True)
    except Unsupported:
        return None
    ground = M._ground_value(prog)
    if ground is not None:
        return unpack(prog, np.zeros((0, 8), np.uint32)) if ground else None
    n = len(prog.leaves)
    soa = E.carry_fill_rungs_host(M.search_leafgen(prog), prog.consts, 0,
                                  np.zeros((n, 8), np.uint32),
                                  np.zeros((1, (n + 31) // 32), np.uint32), SEED, 0,
                                  SEARCH) if n else np.zeros((0, 8, 1), np.uint32)
    hit = np.flatnonzero(evalref.run_leaves_soa(evalref.serialize(nodes, prog), prog, soa))
    return unpack(prog, soa[:, :, int(hit[0])].copy()) if hit.size else None


def crafted_chain():
    """``(queries, known)``: a path that grows one condition at a time — in
    order an extension that hits on "read", three on "all" (one with a fresh
    symbol, one that reads the table at it) and one that misses because its
    parent has come to read the table at a symbolic key — and a group the delta
    refuses: its parent is ``known`` by a witness that is silent about a symbol
    the parent mentions (true whatever that symbol is), as the witness of a
    group that folded to true is."""
    cd, v, u = N.array_var("scd", 256, 8), N.bv_var("sv", 256), N.bv_var("su", 256)
    path = [N.eq(byte(cd, 0), N.bv_num(0xA0, 8)), N.bv_cmp("bvult", v, N.bv_num(100, 256))]
    steps = [N.eq(byte(cd, 2), N.bv_num(0x77, 8)),
             N.bv_cmp("bvult", v, N.bv_num(200, 256)),
             N.bv_cmp("bvugt", u, v),
             N.distinct(N.select(cd, u), N.bv_num(0x55, 8)),
             N.eq(byte(cd, 9), N.bv_num(0x11, 8))]
    out = [list(path)]
    for c in steps:
        out.append(out[-1] + [c])
    w, x = N.bv_var("sw", 256), N.bv_var("sx", 256)
    zero = N.bv_num(0, 256)
    p2 = [N.bv_cmp("bvult", x, N.bv_num(10, 256)),
          N.eq(N.bv_op("bvand", w, zero), N.bv_op("bvand", x, zero))]
    return out + [p2 + [N.bv_cmp("bvugt", w, N.bv_num(5, 256))]], [(p2, Assignment(vars={"sx": 3}))]


def replay(queries, known=()):
    """The queries in order, as model.gpu_search takes them with knob 5 — group
    by group: the memo's plan, the table gate, the delta — on a memo of its own,
    with :func:`cpu_search` where the device would search.  Returns the counts
    and asserts every delta hit on the whole group."""
    memo = CY.HitMemo(1 << 14)
    for nodes, asg in known:
        assert holds(nodes, asg) == []
        memo.note(key_of(nodes), asg)
    st = {"groups": 0, "exact": 0, "eligible": 0, "ineligible": 0, "gated": 0, "hits": [0, 0],
          "missed": 0, "searched": 0, "found": 0}
    for q in queries:
        for group in M.dependence_buckets(list(q)):
            key = key_of(group)
            st["groups"] += 1
            what = CY.plan(key, memo)
            if what is not None and what[0] == "exact":
                st["exact"] += 1
                continue
            if what is not None:
                new = CY.split_nodes(group, what[2])[1]
                if max(CY.table_sizes_ck(new, what[1]).values(), default=0) > CY.MAX_ENTRIES:
                    st["gated"] += 1
                else:
                    (r,) = run_delta([(group, what[1], what[2])])
                    if r is not None and r[0] == "ineligible":
                        st["ineligible"] += 1
                    elif r is not None:
                        st["eligible"] += 1
                        if r[0] is not None:
                            assert holds(group, r[0]) == [], (len(group), len(new), r[3])
                            st["hits"][r[3]] += 1
                            memo.note(key, r[0], r[1])
                            continue
                        st["missed"] += 1
            st["searched"] += 1
            asg = cpu_search(group)
            if asg is not None:
                assert holds(group, asg) == []
                st["found"] += 1
                memo.note(key, asg)
    return st


def test_every_delta_hit_of_a_replayed_stream_satisfies_its_whole_group():
    """The c1 and c4 stand-in streams and the crafted chain.  The host search
    that stands in for the device finds few of the streams' groups (it has no
    solve mode), so the streams give few extensions — c1 one, which hits on
    "all", c4 none — and the chain supplies the rest of the condition."""
    got = {name: replay(W.queries(name, 64)) for name in ("c1", "c4")}
    got["chain"] = replay(*crafted_chain())
    for name, st in got.items():
        print("delta replay %s: %s" % (name, st))
    assert got["chain"]["hits"] == [3, 1] and got["chain"]["missed"] == 1
    assert got["chain"]["ineligible"] == 1 and got["chain"]["eligible"] == 5
    assert got["c1"]["eligible"] >= 1 and got["c1"]["hits"][0] >= 1
    total = {k: sum(np.sum(st[k]) for st in got.values())
             for k in ("eligible", "ineligible", "missed")}
    assert total["eligible"] >= 1 and total["ineligible"] + total["missed"] >= 1
    assert sum(st["hits"][0] for st in got.values()) >= 1

"""Witness sets on the pin ladder, on the host: carry.plan_sets
on hand-made memos, carry.rungs_sets on hand-made groups, the set fill's lane
function (mg_carry_fill_sets_host) against mg_carry_fill_rungs_host rung by rung,
the plan of the device buffer, the merged table sizes, the knob and the gate.
CPU only."""

import numpy as np
import pytest

import census_cases as K
import gen_cases as G
import mythril_amd.model as M
from mythril_amd import carry as CY
from mythril_amd import engine as E
from mythril_amd.assign import Assignment, leaf_values
from mythril_amd.engine import EngineError, default_leafgen
from mythril_amd.smt import node as N

SEED = 0x73657473
FIRST = (1 << 32) + 37                    # above 2^32, no multiple of 64
LADDER = ("ladder", 5)
# case -> (prog_seed, thresholds), as tests/test_gpu_carry_ladder.py runs them
CASES = {LADDER: (3, "default"), "rules": (0, "search"), "flats": (9, "default")}


def asg_of(**values):
    return Assignment(vars=dict(values))


# ---------------------------------------------------------------------------
# plan_sets
# ---------------------------------------------------------------------------

KEY_A, KEY_B, KEY_C = frozenset({1, 2, 3}), frozenset({1, 2, 4}), frozenset({5})
CHILD = frozenset({1, 2, 3, 4, 5, 6})


def abc_memo(size=16):
    """A and B share x (and so conflict), C shares nothing; A is the newest of
    the two of equal size, so ``subsets`` gives A, B, C."""
    memo = CY.HitMemo(size)
    memo.note(KEY_C, asg_of(w=1))
    memo.note(KEY_B, asg_of(x=9, z=1))
    memo.note(KEY_A, asg_of(x=7, y=8))
    return memo


def test_alternative_0_is_plan_and_a_skipped_subset_heads_the_next_alternative():
    memo = abc_memo()
    assert memo.subsets(CHILD) == [KEY_A, KEY_B, KEY_C]
    kind, asg, taken = CY.plan(CHILD, memo)
    what = CY.plan_sets(CHILD, memo)
    assert what[0] == kind == "extend" and len(what[1]) == 2
    assert what[1][0][0].vars == asg.vars == {"x": 7, "y": 8, "w": 1}      # A u C
    assert what[1][0][1] == taken == [KEY_A, KEY_C]
    assert what[1][1][0].vars == {"x": 9, "z": 1, "w": 1}                   # B u C
    assert what[1][1][1] == [KEY_B, KEY_C]
    # pure: the same answer again, the memo unchanged
    before = (dict(memo.hits), dict(memo.seq))
    again = CY.plan_sets(CHILD, memo)
    assert [(a.vars, t) for a, t in again[1]] == [(a.vars, t) for a, t in what[1]]
    assert (dict(memo.hits), dict(memo.seq)) == before
    # one set: plan's answer and nothing else
    (only,) = CY.plan_sets(CHILD, memo, max_sets=1)[1]
    assert only[0].vars == asg.vars and only[1] == taken
    # the default is MAX_SETS, and it is a bound: three pairwise conflicting subsets at 2
    assert CY.MAX_SETS == 4
    for k in range(3):
        memo.note(frozenset({1, 10 + k}), asg_of(x=k))
    assert len(CY.plan_sets(CHILD | {10, 11, 12}, memo, max_sets=2)[1]) == 2
    assert len(CY.plan_sets(CHILD | {10, 11, 12}, memo, max_sets=8)[1]) == 5


def test_exact_none_and_alternatives_without_a_name():
    memo = abc_memo()
    assert CY.plan_sets(KEY_A, memo) == ("exact", memo.hits[KEY_A]) == CY.plan(KEY_A, memo)
    assert CY.plan_sets(frozenset({77, 78}), memo) is None
    # a remembered subset that interprets no name offers nothing, alone or as an alternative
    memo.note(frozenset({6}), Assignment())
    assert CY.plan_sets(frozenset({6, 7}), memo) is None
    alts = CY.plan_sets(CHILD, memo)[1]
    assert len(alts) == 2 and all(CY._names(a) for a, _ in alts)
    assert frozenset({6}) in alts[0][1]


def test_a_bounded_memo_that_dropped_an_entry_does_not_offer_it():
    memo = abc_memo(size=2)                               # C was dropped when A came
    assert KEY_C not in memo.hits and len(memo) == 2
    alts = CY.plan_sets(CHILD, memo)[1]
    assert [(a.vars, t) for a, t in alts] == [({"x": 7, "y": 8}, [KEY_A]),
                                             ({"x": 9, "z": 1}, [KEY_B])]
    memo.note(frozenset({9}), asg_of(q=1))                # drops B
    alts = CY.plan_sets(CHILD, memo)[1]
    assert [(a.vars, t) for a, t in alts] == [({"x": 7, "y": 8}, [KEY_A])]


# ---------------------------------------------------------------------------
# rungs_sets
# ---------------------------------------------------------------------------

def byte(a, k):
    return N.select(a, N.bv_num(k, 256))


def calldata_group(fresh=False):
    """(parent nodes, new nodes) as tests/test_carry_ladder.py builds them: the
    parent fixes calldata bytes 0..3 and bounds a var; the child reads byte 4
    (and, with ``fresh``, compares the var to one of its own)."""
    cd = N.array_var("scd", 256, 8)
    v, u = N.bv_var("sv", 256), N.bv_var("su", 256)
    parent = [N.eq(byte(cd, k), N.bv_num(0xA0 + k, 8)) for k in range(4)]
    parent.append(N.bv_cmp("bvult", v, N.bv_num(100, 256)))
    new = [N.eq(byte(cd, 4), N.bv_num(0x77, 8))]
    if fresh:
        new.append(N.bv_cmp("bvult", v, u))
    return parent, new


def witness(v, n=6):
    return Assignment(vars={"sv": v},
                      arrays={"scd": ([(k, 0xA0 + k & 0xFF) for k in range(n)], 0)})


def bits(mask, n):
    return [bool(int(mask[l >> 5]) >> (l & 31) & 1) for l in range(n)]


def test_the_order_is_rung_major_and_a_repeated_rung_is_dropped():
    parent, new = calldata_group(fresh=True)
    nodes = parent + new
    key = M._group_key(parent)
    alts = [(witness(1), [key]), (witness(2), [key])]
    prog = CY.compile_eval_ck(nodes, alts[0][0], CY.sizes_sets(nodes, alts))
    n = len(prog.leaves)
    rows, masks, rung_set, kept = CY.rungs_sets(prog, alts, nodes)
    assert rows.shape == (2, n, 8) and rows.dtype == masks.dtype == rung_set.dtype == np.uint32
    # "new" frees the table and the var (both occur in the new nodes): it pins nothing, so set
    # 1's repeats set 0's whatever the rows hold
    assert kept == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)]
    assert rung_set.tolist() == [0, 1, 0, 1, 0] and masks.shape == (5, (n + 31) // 32)
    assert not masks[4].any()
    for s, (asg, taken) in enumerate(alts):
        want_rows, ladder = CY.rung_masks(prog, asg, *CY.split_nodes(nodes, taken))
        assert np.array_equal(rows[s], want_rows)
        for i, (r, s2) in enumerate(kept):
            if s2 == s:
                assert np.array_equal(masks[i], ladder[r])
    # the sets differ in the var's row alone, which "all" and "read" pin
    sv = [l.source for l in prog.leaves].index("sv")
    assert [l for l in range(n) if not np.array_equal(rows[0, l], rows[1, l])] == [sv]
    assert bits(masks[0], n)[sv] and bits(masks[2], n)[sv]
    # only pinned rows count: two witnesses that differ where no rung pins collapse entirely
    a, b = witness(1), witness(1)
    b.vars["elsewhere"] = 5
    same = CY.rungs_sets(prog, [(a, [key]), (b, [key])], nodes)
    assert same[3] == [(0, 0), (1, 0), (2, 0)] and same[2].tolist() == [0, 0, 0]
    assert same[0].shape[0] == 2 and (same[2] < same[0].shape[0]).all()


def test_the_list_is_cut_at_eight_rungs_order_kept():
    parent, new = calldata_group()
    nodes = parent + new
    key = M._group_key(parent)
    alts = [(witness(v), [key]) for v in (1, 2, 3)]
    prog = CY.compile_eval_ck(nodes, alts[0][0], CY.sizes_sets(nodes, alts))
    rows, masks, rung_set, kept = CY.rungs_sets(prog, alts, nodes)
    # nine distinct (rung, set) pairs: "new" keeps the var pinned here
    assert kept == [(r, s) for r in range(3) for s in range(3)][:8] and CY.MAX_RUNGS == 8
    assert masks.shape[0] == rung_set.shape[0] == 8 and rows.shape[0] == 3
    assert (rung_set < 3).all() and rung_set.tolist() == [0, 1, 2, 0, 1, 2, 0, 1]
    four = [(witness(v), [key]) for v in (1, 2, 3, 4)]
    assert CY.rungs_sets(prog, four, nodes)[3] == [(0, s) for s in range(4)] + \
        [(1, s) for s in range(4)]


def test_one_alternative_is_rungs():
    for fresh in (False, True):
        parent, new = calldata_group(fresh=fresh)
        nodes = parent + new
        asg, key = witness(1), M._group_key(parent)
        prog = CY.compile_eval_ck(nodes, asg)
        assert prog is CY.compile_eval_ck(nodes, asg, CY.sizes_sets(nodes, [(asg, [key])]))
        rows, masks, rung_set, kept = CY.rungs_sets(prog, [(asg, [key])], nodes)
        want_rows, want_masks = CY.rungs(prog, asg, parent, new)
        assert rows.shape[0] == 1 and np.array_equal(rows[0], want_rows)
        assert np.array_equal(masks, want_masks) and not rung_set.any()
        assert [r for r, _ in kept] == CY.distinct(CY.rung_masks(prog, asg, parent, new)[1])


# ---------------------------------------------------------------------------
# merged sizes
# ---------------------------------------------------------------------------

def test_a_program_at_the_merged_sizes_takes_every_alternatives_leaf_values():
    cd, v = N.array_var("scd", 256, 8), N.bv_var("sv", 256)
    parent, new = calldata_group()
    nodes = parent + [N.eq(N.select(cd, v), N.bv_num(0xA1, 8))] + new      # a symbolic read
    small, big = witness(1, n=6), witness(2, n=12)
    assert CY.table_sizes_ck(nodes, small) == {"scd": 2}
    assert CY.table_sizes_ck(nodes, big) == {"scd": 7}                     # 12 less keys 0..4
    alts = [(small, []), (big, [])]
    assert CY.sizes_sets(nodes, alts) == {"scd": 7} == CY.sizes_sets(nodes, alts[::-1])
    with pytest.raises(ValueError):                        # alternative 0's own sizes do not fit
        leaf_values(CY.compile_eval_ck(nodes, small), big)
    prog = CY.compile_eval_ck(nodes, small, CY.sizes_sets(nodes, alts))
    assert prog.table_sizes["scd"] == 7
    for asg, _ in alts:
        assert len(leaf_values(prog, asg)) == len(prog.leaves)
    rows = CY.rungs_sets(prog, [(small, [M._group_key(parent)]), (big, [M._group_key(parent)])],
                         nodes)[0]
    assert rows.shape == (2, len(prog.leaves), 8)


# ---------------------------------------------------------------------------
# the lane function
# ---------------------------------------------------------------------------

def built(case):
    if isinstance(case, tuple):
        return K.masked_program(case)[1]
    return G.program(case, 16, "mask")


def random_sets(prog, seed, n_rungs, n_sets, share):
    rng = np.random.default_rng(seed)
    n = len(prog.leaves)
    masks = np.zeros((n_rungs, (n + 31) // 32), dtype=np.uint32)
    rows = np.zeros((n_sets, n, 8), dtype=np.uint32)
    for l, leaf in enumerate(prog.leaves):
        for s in range(n_sets):
            v = int.from_bytes(rng.bytes(32), "little") & ((1 << leaf.width) - 1)
            rows[s, l] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
        for r in range(n_rungs):
            if rng.random() < share:
                masks[r, l >> 5] |= np.uint32(1 << (l & 31))
    rung_set = rng.integers(0, n_sets, size=n_rungs).astype(np.uint32)
    rung_set[rng.integers(0, n_rungs)] = n_sets - 1       # the last set is in use
    return masks, rows, rung_set


@pytest.mark.parametrize("lanes", (1, 63, 65))
@pytest.mark.parametrize("case,n_rungs,n_sets", (("flats", 2, 3), ("rules", 4, 3), (LADDER, 3, 2)))
def test_every_rung_is_fill_rungs_host_with_that_rungs_row_set(case, n_rungs, n_sets, lanes):
    prog = built(case)
    n = len(prog.leaves)
    assert n == {"flats": 274, "rules": 15, LADDER: 3}[case]
    gens = M.search_leafgen(prog) if CASES[case][1] == "search" else default_leafgen(prog)
    masks, rows, rung_set = random_sets(prog, 7 * n + lanes, n_rungs, n_sets, 0.5)
    if case == "flats":
        assert masks[:, 1:].any()                          # pinned leaves past mask word 0
    assert len({rows[s].tobytes() for s in range(n_sets)}) == n_sets
    ps = CASES[case][0]
    cols = (n_rungs + 1) * lanes                           # a surplus rung repeats the last
    out = E.carry_fill_sets_host(gens, prog.consts, ps, rows, masks, rung_set, SEED, FIRST, lanes,
                                 cols=cols)
    assert out.shape == (n, 8, cols)
    pinned_somewhere = False
    for r in range(n_rungs + 1):
        q = min(r, n_rungs - 1)
        want = E.carry_fill_rungs_host(gens, prog.consts, ps, rows[rung_set[q]], masks[q:q + 1],
                                       SEED, FIRST, lanes)
        assert np.array_equal(out[:, :, r * lanes:(r + 1) * lanes], want), (case, r, lanes)
        other = E.carry_fill_rungs_host(gens, prog.consts, ps, rows[(rung_set[q] + 1) % n_sets],
                                        masks[q:q + 1], SEED, FIRST, lanes)
        pinned_somewhere |= not np.array_equal(other, want)
    assert pinned_somewhere                                # the row set matters
    # a column range across a rung boundary is a slice
    if lanes > 1:
        part = E.carry_fill_sets_host(gens, prog.consts, ps, rows, masks, rung_set, SEED, FIRST,
                                      lanes, cols=cols, col0=lanes - 1, n_cols=2)
        assert np.array_equal(part, out[:, :, lanes - 1:lanes + 1])


def test_fill_sets_host_refusals():
    prog = built(LADDER)
    gens = default_leafgen(prog)
    masks, rows, rung_set = random_sets(prog, 1, 2, 2, 0.5)
    E.carry_fill_sets_host(gens, prog.consts, 0, rows, masks, rung_set, 0, 0, 4)
    with pytest.raises(EngineError):                       # a rung of set 2 of 2
        E.carry_fill_sets_host(gens, prog.consts, 0, rows, masks, [0, 2], 0, 0, 4)
    with pytest.raises(EngineError):                       # 9 sets
        E.carry_fill_sets_host(gens, prog.consts, 0, np.zeros((9, 3, 8), dtype=np.uint32), masks,
                               rung_set, 0, 0, 4)
    with pytest.raises(EngineError):                       # none
        E.carry_fill_sets_host(gens, prog.consts, 0, np.zeros((0, 3, 8), dtype=np.uint32), masks,
                               [0, 0], 0, 0, 4)
    with pytest.raises(EngineError):                       # 9 rungs
        E.carry_fill_sets_host(gens, prog.consts, 0, rows, np.zeros((9, 1), dtype=np.uint32),
                               [0] * 9, 0, 0, 4)
    for lanes, cols, col0, n_cols in ((0, 8, 0, 1), (4, 2, 0, 1), (4, (1 << 20) + 1, 0, 1),
                                      (4, 8, 9, 0), (4, 8, 6, 3)):
        with pytest.raises(EngineError):
            E.carry_fill_sets_host(gens, prog.consts, 0, rows, masks, rung_set, 0, 0, lanes, cols,
                                   col0, n_cols)
    for bad in ((rows[0], masks, rung_set), (rows, masks[0], rung_set), (rows, masks, [0])):
        with pytest.raises(ValueError):
            E.carry_fill_sets_host(gens, prog.consts, 0, *bad, 0, 0, 4)


# ---------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------

def test_sets_plan_is_the_ladders_with_row_sets_records_and_rung_sets():
    counts, n_rungs, n_sets = [3, 274, 0, 15], [3, 1, 8, 4], [2, 1, 8, 3]
    lanes, max_leaves = 65, 300
    off, total, stride = E.carry_sets_plan_host(counts, n_rungs, n_sets, lanes, max_leaves)
    n, cols = len(counts), 8 * lanes
    base = E.CARRY_SHARED + n * E.CARRY_JOB_REGIONS
    assert len(off) == base + E.CARRY_SETS_SHARED + n * E.CARRY_SETS_JOB_REGIONS
    assert all(int(o) % 256 == 0 for o in off) and total % 256 == 0

    def up(b):
        return (b + 255) // 256 * 256
    descs, jobs, first, out = (int(o) for o in off[:4])
    per = np.asarray(off[4:base], dtype=np.uint64).reshape(n, 4).astype(object)
    records, sets = int(off[base]), [int(o) for o in off[base + 1:]]
    order = [descs, jobs, first] + [int(per[g][k]) for g in range(n) for k in range(3)] + \
        [records] + sets + [out] + [int(per[g][3]) for g in range(n)] + [total]
    assert order == sorted(order) and order[0] == 0
    for g, (k, r, s) in enumerate(zip(counts, n_rungs, n_sets)):
        assert int(per[g][1]) - int(per[g][0]) == up((k + 31) // 32 * 4 * r)
        assert int(per[g][2]) - int(per[g][1]) == up(s * k * 32)           # n_sets row sets
        nxt = int(per[g + 1][0]) if g + 1 < n else records
        assert nxt - int(per[g][2]) == up(k * 24)
        assert (sets[g + 1] if g + 1 < n else out) - sets[g] == up(r * 4)
    assert sets[0] - records == up(n * 16)                                 # one record per job
    assert int(per[0][3]) - out == up(n * (16 + max_leaves * 32))
    want = up(274 * 8 * cols * 4)
    assert stride * 4 == want and total == int(per[0][3]) + n * want
    assert [int(per[g][3]) for g in range(n)] == [int(per[0][3]) + g * want for g in range(n)]
    # one set each: the ladder's uploaded front at the ladder's own offsets, the same stride
    a = E.carry_sets_plan_host(counts, n_rungs, [1] * n, lanes, max_leaves)
    b = E.carry_ladder_plan_host(counts, n_rungs, lanes, max_leaves)
    assert a[2] == b[2] and np.array_equal(a[0][:3], b[0][:3])
    assert np.array_equal(np.asarray(a[0][4:base]).reshape(n, 4)[:, :3],
                          np.asarray(b[0][4:]).reshape(n, 4)[:, :3])
    assert int(a[0][base]) == int(b[0][3])                 # the records lie where its output lay


def test_sets_plan_refusals():
    E.carry_sets_plan_host([1], [1], [1], 1, 1)
    E.carry_sets_plan_host([1] * 256, [8] * 256, [8] * 256, 1 << 17, 1)
    for counts, n_rungs, n_sets, lanes in (
            ([], [], [], 4), ([1] * 257, [1] * 257, [1] * 257, 4), ([1], [1], [1], 0),
            ([1], [1], [1], (1 << 20) + 1), ([1], [0], [1], 4), ([1], [9], [1], 4),
            ([1], [1], [0], 4), ([1], [1], [9], 4), ([1, 1], [1, 1], [1, 9], 4),
            ([1, 1], [1, 2], [1, 1], (1 << 19) + 1), ([1], [8], [1], (1 << 17) + 1)):
        with pytest.raises(EngineError):
            E.carry_sets_plan_host(counts, n_rungs, n_sets, lanes, 1)
    with pytest.raises(EngineError):                       # beyond 64 bits
        E.carry_sets_plan_host([0xFFFFFFFF] * 256, [8] * 256, [8] * 256, 1 << 17, 1)
    with pytest.raises(ValueError):
        E.carry_sets_plan_host([1, 1], [1, 1], [1], 4, 1)


# ---------------------------------------------------------------------------
# the knob and the gate
# ---------------------------------------------------------------------------

def test_knob_4_selects_the_sets_and_the_statistics_show_set_hits_only_past_set_0(monkeypatch):
    monkeypatch.setattr(CY, "MAX_SETS", CY.MAX_SETS)       # put back whatever the env sets
    try:
        M.configure_from_env({"MYTHRIL_GPU_CARRY": "4"})
        assert M.CARRY == "sets" and CY.MAX_SETS == 4
        for text, want in (("0", 1), ("3", 3), ("8", 8), ("99", 8)):
            M.configure_from_env({"MYTHRIL_GPU_CARRY": "4", "MYTHRIL_GPU_CARRY_SETS": text})
            assert CY.MAX_SETS == want
        assert len(M.SolverStatistics().carry_set_hits) == 8
        for text, want in (("2", "ladder"), ("3", "walk"), ("1", True), ("0", False)):
            M.configure_from_env({"MYTHRIL_GPU_CARRY": text})
            assert M.CARRY == want
    finally:
        M.configure_from_env()
    assert M.CARRY is False
    monkeypatch.setattr(CY, "MAX_SETS", 4)
    s = M.SolverStatistics()
    assert s.carry_set_hits == [0, 0, 0, 0]
    s.carry_attempts, s.carry_hits, s.carry_candidates = 2, 1, 513
    s.carry_rung_hits[0] += 1
    s.carry_set_hits[0] += 1
    assert repr(s).endswith("candidates: 513 rung hits: 1/0/0")            # as under knob 2
    s.carry_set_hits[1] += 1
    assert repr(s).endswith("candidates: 513 rung hits: 1/0/0 set hits: 1/1/0/0")
    s.reset_gpu()
    assert s.carry_set_hits == [0, 0, 0, 0]


def test_knob_4_hands_run_sets_the_alternatives_and_gates_on_the_merged_sizes(monkeypatch):
    cd, v = N.array_var("scd", 256, 8), N.bv_var("sv", 256)
    parent, new = calldata_group()
    sym = N.eq(N.select(cd, v), N.bv_num(0xA1, 8))
    other = parent[:4] + [sym]                             # shares the table with the parent
    nodes = parent + [sym] + new
    M.clear_search_memos()
    M.stats.reset_gpu()
    seen = []

    def fake(eng, items, seed, leafgen, lanes=None, phase=None):
        seen.extend(items)
        return [None] * len(items)
    monkeypatch.setattr(CY, "run_sets", fake)
    try:
        monkeypatch.setattr(M, "CARRY", "sets")
        M._note_hit(M._group_key(other), witness(1, n=6))
        M._note_hit(M._group_key(parent), witness(2, n=6))
        assert M._carry_groups([(M._group_key(nodes), nodes)], eng=object()) == {}
        s = M.stats
        assert (s.carry_gated, s.carry_attempts) == (0, 0)
        (item,) = seen
        assert item[0] == nodes and [t for _, t in item[1]] == \
            [[M._group_key(parent)], [M._group_key(other)]]
        # alternative 1 alone holds a table above the cap: the group is gated, nothing runs
        M.clear_search_memos()
        M._note_hit(M._group_key(other), witness(1, n=68))
        M._note_hit(M._group_key(parent), witness(2, n=6))
        assert CY.table_sizes_ck(nodes, witness(2, n=6))["scd"] <= CY.MAX_ENTRIES
        assert M._carry_groups([(M._group_key(nodes), nodes)], eng=object()) == {}
        assert (s.carry_gated, s.carry_attempts) == (1, 0) and len(seen) == 1
    finally:
        M.clear_search_memos()
        M.stats.reset_gpu()

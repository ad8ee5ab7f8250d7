"""Witness carry on the host: the fill kernel's lane function
(mg_carry_fill_host, csrc/mg_carry.h) against the oracle's generator
(oracle/gen_ref.py), carry.pins against assign.leaf_values, the pin-set rule
and the hit memo, the plan of the batch's device buffer, and the knob.  CPU
only."""

import numpy as np
import pytest

import mythril_amd.model as M
from mythril_amd import carry as CY
from mythril_amd import engine as E
from mythril_amd.assign import Assignment, leaf_values
from mythril_amd.engine import EngineError, LeafGen
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N
from oracle import gen_ref

WIDTHS = (1, 8, 32, 33, 64, 160, 256)
POOL = (0, (1 << 256) - 1, 0x1234, (1 << 160) + 5, 1 << 255)
PCTS = ((20, 40, 60), (50, 70, 85))
SEED, PROG_SEED = 0x63617272, 0x5EED
# ranges that cross a multiple of 64, and that lie above 2^32
FIRSTS = (0, 40, (1 << 32) + 37, (1 << 40) + 64 - 9)
LANES = 200


def rows_of(values):
    return np.stack([np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u4") for v in values])


def ints_of(col):
    return [int.from_bytes(np.ascontiguousarray(r, dtype="<u4").tobytes(), "little") for r in col]


def consts_with_pool():
    c = np.zeros((2 + len(POOL), 8), dtype=np.uint32)
    c[2:] = rows_of(POOL)
    return c


@pytest.mark.parametrize("pct", PCTS)
@pytest.mark.parametrize("pool_n", (0, 1, 5))
def test_free_leaves_equal_the_oracle_generator(pct, pool_n):
    gens = [LeafGen(w, 2, pool_n, *pct) for w in WIDTHS]
    n = len(WIDTHS)
    mask, rows = np.zeros(1, dtype=np.uint32), np.zeros((n, 8), dtype=np.uint32)
    seen = set()
    for first in FIRSTS:
        out, cls = E.carry_fill_host(gens, consts_with_pool(), PROG_SEED, rows, mask, SEED, first,
                                     LANES, want_classes=True)
        assert out.shape == (n, 8, LANES)
        seen |= set(np.unique(cls).tolist())
        for l, w in enumerate(WIDTHS):
            got = ints_of(out[l].T)
            want = [gen_ref.gen_leaf(SEED, PROG_SEED, l, first + i, w, POOL[:pool_n], pct)
                    for i in range(LANES)]
            assert got == want, (pct, pool_n, first, w)
            assert all(v >> w == 0 for v in got)
    # every generator class occurs in the sample (no pool: its class is uniform)
    assert seen == ({0, 1, 2, 3} if pool_n else {0, 1, 3})


def test_a_lane_range_is_a_slice_of_the_whole():
    gens = [LeafGen(w, 2, 5, 20, 40, 60) for w in WIDTHS]
    mask, rows = np.zeros(1, dtype=np.uint32), np.zeros((len(WIDTHS), 8), dtype=np.uint32)
    whole = E.carry_fill_host(gens, consts_with_pool(), PROG_SEED, rows, mask, SEED, FIRSTS[2], 130)
    part = E.carry_fill_host(gens, consts_with_pool(), PROG_SEED, rows, mask, SEED, FIRSTS[2], 130,
                             lane0=61, n_lanes=8)
    assert np.array_equal(part, whole[:, :, 61:69])


def test_pinned_leaves_are_their_rows_on_every_lane_past_mask_bit_31():
    n = 40
    widths = [WIDTHS[i % len(WIDTHS)] for i in range(n)]
    gens = [LeafGen(w, 2, 5, 20, 40, 60) for w in widths]
    rng = np.random.default_rng(7)
    vals = [int.from_bytes(rng.bytes(32), "little") & ((1 << w) - 1) for w in widths]
    rows = rows_of(vals)
    pinned = {0, 3, 31, 32, 33, 39}
    mask = np.zeros(2, dtype=np.uint32)
    for l in pinned:
        mask[l >> 5] |= np.uint32(1 << (l & 31))
    out, cls = E.carry_fill_host(gens, consts_with_pool(), PROG_SEED, rows, mask, SEED, FIRSTS[3],
                                 70, want_classes=True)
    for l in range(n):
        if l in pinned:
            assert np.array_equal(out[l], np.repeat(rows[l][:, None], 70, axis=1)), l
            assert (cls[l] == 0xFFFFFFFF).all()
        else:
            want = [gen_ref.gen_leaf(SEED, PROG_SEED, l, FIRSTS[3] + i, widths[l], POOL,
                                     (20, 40, 60)) for i in range(70)]
            assert ints_of(out[l].T) == want, l


def test_fill_host_refusals():
    mask, rows = np.zeros(1, dtype=np.uint32), np.zeros((1, 8), dtype=np.uint32)
    c = consts_with_pool()
    ok = [LeafGen(8, 2, 5, 20, 40, 60)]
    E.carry_fill_host(ok, c, 0, rows, mask, 0, 0, 4)
    for bad in ([LeafGen(0, 0, 0, 20, 40, 60)], [LeafGen(257, 0, 0, 20, 40, 60)],
                [LeafGen(8, 3, 5, 20, 40, 60)], [LeafGen(8, 0xFFFFFFFF, 2, 20, 40, 60)]):
        with pytest.raises(EngineError):
            E.carry_fill_host(bad, c, 0, rows, mask, 0, 0, 4)
    for lanes, lane0, n_lanes in ((0, 0, 0), ((1 << 20) + 1, 0, 1), (4, 4, 1), (4, 2, 3)):
        with pytest.raises(EngineError):
            E.carry_fill_host(ok, c, 0, rows, mask, 0, 0, lanes, lane0, n_lanes or 1)


# ---------------------------------------------------------------------------
# carry.pins
# ---------------------------------------------------------------------------

def _group():
    x, y = N.bv_var("cx", 256), N.bv_var("cy", 64)
    wide = N.bv_var("cw", 512)
    a, b = N.array_var("ca", 256, 256), N.array_var("cb", 256, 256)
    cs = [N.eq(N.select(a, x), N.bv_num(5, 256)),
          N.bv_cmp("bvult", y, N.bv_num(100, 64)),
          N.eq(N.select(b, N.bv_num(1, 256)), x),
          N.eq(N.extract(300, 300, wide), N.bv_num(1, 1))]
    return cs


def test_pins_follow_leaf_values_and_leave_fresh_symbols_free():
    cs = _group()
    asg = Assignment(vars={"cx": 7, "cw": (1 << 300) | 5},
                     arrays={"ca": ([(7, 5), (9, 11)], 3)})
    prog = CY.compile_eval(cs, asg)
    mask, rows = CY.pins(prog, asg)
    vals = leaf_values(prog, asg)
    assert mask.shape == ((len(prog.leaves) + 31) // 32,) and rows.shape == (len(prog.leaves), 8)
    kinds = set()
    for l, leaf in enumerate(prog.leaves):
        bit = bool(mask[l >> 5] >> (l & 31) & 1)
        assert bit == (leaf.source in ("cx", "cw", "ca")), leaf
        if bit:
            assert ints_of([rows[l]])[0] == vals[l] and vals[l] >> leaf.width == 0
            kinds.add((leaf.source, leaf.chunk))
        else:
            assert not rows[l].any()
    # a fresh var and a fresh array are free; a var wider than a chunk is pinned per chunk
    assert {l.source for l in prog.leaves} >= {"cy", "cb"}
    assert ("cw", 0) in kinds and ("cw", 1) in kinds
    assert CY.n_free(prog, mask) == sum(l.source in ("cy", "cb") for l in prog.leaves) > 0


def test_a_carried_table_larger_than_the_default_enlarges_the_program():
    cs = _group()
    entries = [(k, k + 100) for k in range(5)]
    asg = Assignment(vars={"cx": 2}, arrays={"ca": (entries, 9)})
    assert CY.table_sizes(asg) == {"ca": 5} and CY.DEFAULT_ENTRIES == 2
    assert CY.table_sizes(Assignment(arrays={"ca": ([(1, 1)], 0)})) == {"ca": 2}
    prog = CY.compile_eval(cs, asg)
    assert prog.table_sizes["ca"] == 5 and prog.table_sizes["cb"] == 2
    assert prog is CY.compile_eval(cs, asg)                       # cached
    assert compile_constraints(cs, leaf_pools=True).table_sizes["ca"] == 2
    mask, rows = CY.pins(prog, asg)
    vals = leaf_values(prog, asg)
    mine = [l for l, leaf in enumerate(prog.leaves) if leaf.source == "ca"]
    assert len(mine) >= 2 * 5
    for l in mine:
        assert mask[l >> 5] >> (l & 31) & 1
        assert ints_of([rows[l]])[0] == vals[l]
    keys = {vals[l] for l in mine if prog.leaves[l].kind == "key"}
    assert keys == {0, 1, 2, 3, 4}


# ---------------------------------------------------------------------------
# the pin-set rule and the memo
# ---------------------------------------------------------------------------

def fs(*ids):
    return frozenset(ids)


def test_largest_subset_first_newest_among_equals_and_the_conflict_skip():
    memo = CY.HitMemo(16)
    memo.note(fs(1), Assignment(vars={"a": 1}))
    memo.note(fs(1, 2), Assignment(vars={"a": 2, "b": 2}))
    memo.note(fs(3), Assignment(vars={"c": 3}))
    memo.note(fs(4), Assignment(vars={"c": 4}))                 # newer than {3}, same size
    memo.note(fs(5, 9), Assignment(vars={"z": 1}))              # no subset of the key
    key = fs(1, 2, 3, 4, 5)
    assert memo.subsets(key) == [fs(1, 2), fs(4), fs(3), fs(1)]
    what = CY.plan(key, memo)
    assert what[0] == "extend"
    # {1} conflicts with {1, 2} on a, {3} with the newer {4} on c
    assert what[2] == [fs(1, 2), fs(4)]
    assert what[1].vars == {"a": 2, "b": 2, "c": 4}
    # deterministic: the same key and memo give the same plan, whatever the order asked
    again = CY.plan(frozenset(sorted(key, reverse=True)), memo)
    assert again[2] == what[2] and again[1].vars == what[1].vars
    # tables conflict by name too
    memo.note(fs(6), Assignment(arrays={"t": ([(1, 1)], 0)}))
    memo.note(fs(7), Assignment(funcs={"t": ([(2, 2)], 0)}, vars={"q": 1}))
    w2 = CY.plan(fs(6, 7, 8), memo)
    assert w2[2] == [fs(7)] and "t" in w2[1].funcs and not w2[1].arrays


def test_an_exact_key_short_circuits_and_a_stranger_gets_nothing():
    memo = CY.HitMemo(16)
    a = Assignment(vars={"a": 1})
    memo.note(fs(1, 2), a)
    memo.note(fs(1), Assignment(vars={"a": 9}))
    assert CY.plan(fs(1, 2), memo) == ("exact", a)
    assert CY.plan(fs(2, 3), memo) is None
    assert CY.plan(fs(1), memo)[0] == "exact"
    # a remembered group with nothing to pin (a ground group) gives no pin set
    memo.note(fs(8), Assignment())
    assert CY.plan(fs(8, 9), memo) is None


def test_the_memo_is_bounded_and_cleared(monkeypatch):
    memo = CY.HitMemo(4)
    for k in range(10):
        memo.note(fs(k, 100), Assignment(vars={"v": k}))
    assert len(memo) == 4 and list(memo.hits) == [fs(k, 100) for k in range(6, 10)]
    assert sorted(memo.index) == [6, 7, 8, 9] and len(memo.seq) == 4
    assert CY.plan(fs(0, 100, 200), memo) is None                # dropped with the oldest
    assert CY.plan(fs(9, 100, 7), memo)[2] == [fs(9, 100)]
    # model.py's memo: filled only with the knob on, bounded like the miss memo
    M.clear_search_memos()
    monkeypatch.setattr(M, "CARRY", False)
    M._note_hit(fs(1), Assignment(vars={"a": 1}))
    assert not M._group_hit
    monkeypatch.setattr(M, "CARRY", True)
    monkeypatch.setattr(M, "GROUP_MISS_SIZE", 3)
    for k in range(5):
        M._note_hit(fs(k), Assignment(vars={"a": k}))
    assert list(M._group_hit) == [fs(2), fs(3), fs(4)] and sorted(M._hit_index) == [2, 3, 4]
    M.clear_search_memos()
    assert not M._group_hit and not M._hit_index and not CY._EVAL_CACHE


# ---------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------

def test_plan_regions_are_aligned_in_order_and_strided_by_the_maximum():
    counts, lanes, max_leaves = [3, 40, 0, 17], 65, 41
    off, total, stride = E.carry_plan_host(counts, lanes, max_leaves)
    n = len(counts)
    assert len(off) == E.CARRY_SHARED + n * E.CARRY_JOB_REGIONS
    assert all(int(o) % 256 == 0 for o in off) and total % 256 == 0
    descs, jobs, first, out = (int(o) for o in off[:4])
    per = np.asarray(off[4:], dtype=np.uint64).reshape(n, 4).astype(object)
    order = [descs, jobs, first] + [int(per[g][k]) for g in range(n) for k in range(3)] + [out] + \
        [int(per[g][3]) for g in range(n)] + [total]
    assert order == sorted(order) and order[0] == 0
    # sizes: the regions are as large as what is written into them
    assert first - jobs >= n * 48 and int(per[0][0]) - first >= n * 8
    for g, k in enumerate(counts):
        assert int(per[g][1]) - int(per[g][0]) >= (k + 31) // 32 * 4
        assert int(per[g][2]) - int(per[g][1]) >= k * 32
    assert int(per[0][3]) - out >= n * (8 + max_leaves * 32)
    # the leaf stride is the batch maximum, rounded up to 256 bytes
    want = (40 * 8 * lanes * 4 + 255) // 256 * 256
    assert stride * 4 == want
    assert [int(per[g][3]) for g in range(n)] == [int(per[0][3]) + g * want for g in range(n)]
    assert total == int(per[0][3]) + n * want


def test_plan_refusals():
    E.carry_plan_host([1], 1, 1)
    E.carry_plan_host([1] * 256, 1 << 20, 1)
    for counts, lanes in (([], 4), ([1] * 257, 4), ([1], 0), ([1], (1 << 20) + 1)):
        with pytest.raises(EngineError):
            E.carry_plan_host(counts, lanes, 1)
    # 256 regions of 2^32 - 1 leaves x 32 bytes x 2^20 lanes: beyond 64 bits
    with pytest.raises(EngineError):
        E.carry_plan_host([0xFFFFFFFF] * 256, 1 << 20, 1)
    off, total, stride = E.carry_plan_host([0xFFFFFFFF] * 2, 1 << 20, 1)
    assert total > 1 << 57


# ---------------------------------------------------------------------------
# the knob
# ---------------------------------------------------------------------------

PARENT_REPR = ("Query count: 0 \nSolver time: 0.0\n"
               "GPU pre-filter: queries: 0 hits: 0 fallbacks: 0 unsupported: 0 errors: 0 "
               "rejected by z3: 0 memo misses: 0 compile-gated: 0 shape-skipped: 0 refuted: 0\n"
               "GPU candidates: 0 time: 0.000s (kernel 0.000s; flatten 0.000s, refute 0.000s, "
               "compile 0.000s, load 0.000s, search 0.000s, verify 0.000s)")


def test_knob_off_by_default_and_the_statistics_line_is_unchanged():
    lanes = CY.CARRY_LANES
    try:
        M.configure_from_env({})
        assert M.CARRY is False and CY.CARRY_LANES == lanes
        assert repr(M.SolverStatistics()) == PARENT_REPR
        M.configure_from_env({"MYTHRIL_GPU_CARRY": "1", "MYTHRIL_GPU_CARRY_LANES": "1024"})
        assert M.CARRY is True and CY.CARRY_LANES == 1024
        s = M.SolverStatistics()
        s.carry_exact, s.carry_attempts, s.carry_hits, s.carry_candidates = 3, 2, 1, 257
        assert repr(s) == PARENT_REPR + "\nGPU carry: exact: 3 attempts: 2 hits: 1 candidates: 257"
    finally:
        CY.CARRY_LANES = lanes
        M.configure_from_env()
    assert M.CARRY is False


def test_knob_off_the_empty_query_takes_the_parent_route(monkeypatch):
    # no group at all: the shortcut for "every group carried" must not fire with
    # nothing carried; the parent's gpu_search fails on the empty group list and
    # get_model falls back, and so does this one
    monkeypatch.setattr(M, "CARRY", False)
    M.clear_search_memos()
    with pytest.raises(IndexError):
        M.gpu_search([], 100.0)
    monkeypatch.setattr(M, "CARRY", True)
    with pytest.raises(IndexError):
        M.gpu_search([], 100.0)


def test_a_carried_table_above_the_cap_is_not_carried_and_only_jobs_that_ran_count(monkeypatch):
    from mythril_amd.ir import Unsupported
    monkeypatch.setattr(M, "CARRY", True)
    M.clear_search_memos()
    M.stats.reset_gpu()
    cs = _group()
    keys = [M._group_key([c]) for c in cs]
    big = Assignment(vars={"cx": 1}, arrays={"ca": ([(k, k) for k in range(CY.MAX_ENTRIES + 1)], 0)})
    M._note_hit(keys[0], big)
    # the extension's pin set holds a table of MAX_ENTRIES + 1 entries: gated, no engine needed
    assert M._carry_groups([(M._group_key(cs[:2]), cs[:2])], eng=None) == {}
    assert (M.stats.carry_gated, M.stats.carry_attempts, M.stats.kernel_calls) == (1, 0, 0)
    assert "table-gated: 1" in repr(M.stats)
    # at the cap it is a job; one whose eval form is unsupported did not run and is no attempt
    M.clear_search_memos()
    M.stats.reset_gpu()
    ok = Assignment(vars={"cx": 1}, arrays={"ca": ([(k, k) for k in range(CY.MAX_ENTRIES)], 0)})
    M._note_hit(keys[0], ok)

    def refuse(nodes, asg):
        raise Unsupported("no eval form")
    monkeypatch.setattr(CY, "compile_eval", refuse)
    assert M._carry_groups([(M._group_key(cs[:2]), cs[:2])], eng=object()) == {}
    assert (M.stats.carry_gated, M.stats.carry_attempts, M.stats.kernel_calls,
            M.stats.launches) == (0, 0, 0, 0)
    M.clear_search_memos()
    M.stats.reset_gpu()


def test_launch_counts_of_a_search():
    class P:
        solved = False
    assert M._search_launches(1 << 20) == 2                    # batched: search + regeneration
    assert M._search_launches((1 << 26) + 1) == 3
    assert M._search_launches(1 << 20, (-1, P)) == 1           # Engine.search, a miss
    assert M._search_launches(1 << 20, (5, P)) == 2            # a hit: its witness regenerated
    P.solved = True
    assert M._search_launches(1 << 20, (5, P)) == 3            # and re-evaluated for its probes

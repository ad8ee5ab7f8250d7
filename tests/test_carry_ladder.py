"""The pin ladder of the witness carry on the host: the rung
fill's lane function (mg_carry_fill_rungs_host) against mg_carry_fill_host rung
by rung, the plan of the ladder's device buffer, carry.rungs and
carry.compile_eval_ck on hand-made groups, the oracle on the pinned rows, and
the knob.  CPU only."""

import numpy as np
import pytest

import mythril_amd.model as M
from mythril_amd import carry as CY
from mythril_amd import engine as E
from mythril_amd.assign import Assignment, leaf_values
from mythril_amd.engine import EngineError, LeafGen
from mythril_amd.smt import node as N
from oracle import evalref

WIDTHS = (1, 8, 32, 33, 64, 160, 256)
POOL = (0, (1 << 256) - 1, 0x1234, (1 << 160) + 5, 1 << 255)
SEED, PROG_SEED = 0x6C616464, 0x5EED
FIRST = (1 << 32) + 37


def rows_of(values):
    return np.stack([np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u4") for v in values])


def consts_with_pool():
    c = np.zeros((2 + len(POOL), 8), dtype=np.uint32)
    c[2:] = rows_of(POOL)
    return c


def bit(mask, l):
    return bool(int(mask[l >> 5]) >> (l & 31) & 1)


def random_job(n, n_rungs, seed):
    rng = np.random.default_rng(seed)
    widths = [WIDTHS[i % len(WIDTHS)] for i in range(n)]
    gens = [LeafGen(w, 2, 5, 20, 40, 60) for w in widths]
    rows = rows_of([int.from_bytes(rng.bytes(32), "little") for _ in range(n)])
    masks = rng.integers(0, 1 << 32, size=(n_rungs, (n + 31) // 32), dtype=np.uint64)
    return gens, rows, masks.astype(np.uint32)


# ---------------------------------------------------------------------------
# the lane function
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", (1, 63, 64, 65, 256))
def test_every_rung_is_fill_host_under_that_rungs_mask(lanes):
    c = consts_with_pool()
    for n, n_rungs in ((3, 3), (40, 1), (15, 2), (7, 8)):
        gens, rows, masks = random_job(n, n_rungs, 100 * n + n_rungs)
        out = E.carry_fill_rungs_host(gens, c, PROG_SEED, rows, masks, SEED, FIRST, lanes)
        assert out.shape == (n, 8, n_rungs * lanes)
        for r in range(n_rungs):
            want = E.carry_fill_host(gens, c, PROG_SEED, rows, masks[r], SEED, FIRST, lanes)
            assert np.array_equal(out[:, :, r * lanes:(r + 1) * lanes], want), (n, r, lanes)


def test_a_job_with_fewer_rungs_repeats_its_last_rung_and_a_range_is_a_slice():
    c, lanes, R = consts_with_pool(), 65, 3
    for n_rungs in (1, 2):
        gens, rows, masks = random_job(40, n_rungs, n_rungs)
        out = E.carry_fill_rungs_host(gens, c, PROG_SEED, rows, masks, SEED, FIRST, lanes,
                                      cols=R * lanes)
        assert out.shape == (40, 8, R * lanes)
        for r in range(R):
            want = E.carry_fill_host(gens, c, PROG_SEED, rows, masks[min(r, n_rungs - 1)], SEED,
                                     FIRST, lanes)
            assert np.array_equal(out[:, :, r * lanes:(r + 1) * lanes], want), (n_rungs, r)
        # a column range across a rung boundary
        part = E.carry_fill_rungs_host(gens, c, PROG_SEED, rows, masks, SEED, FIRST, lanes,
                                       cols=R * lanes, col0=60, n_cols=11)
        assert np.array_equal(part, out[:, :, 60:71])


def test_fill_rungs_host_refusals():
    c = consts_with_pool()
    gens, rows, masks = random_job(3, 2, 5)
    E.carry_fill_rungs_host(gens, c, 0, rows, masks, 0, 0, 4)
    with pytest.raises(EngineError):                           # 9 rungs
        E.carry_fill_rungs_host(gens, c, 0, rows, np.zeros((9, 1), dtype=np.uint32), 0, 0, 4)
    with pytest.raises(EngineError):                           # none
        E.carry_fill_rungs_host(gens, c, 0, rows, np.zeros((0, 1), dtype=np.uint32), 0, 0, 4)
    for lanes, cols, col0, n_cols in ((0, 8, 0, 1), (4, 2, 0, 1), (4, (1 << 20) + 1, 0, 1),
                                      (4, 8, 9, 0), (4, 8, 6, 3)):
        with pytest.raises(EngineError):
            E.carry_fill_rungs_host(gens, c, 0, rows, masks, 0, 0, lanes, cols, col0, n_cols)
    with pytest.raises(EngineError):
        E.carry_fill_rungs_host([LeafGen(0, 0, 0, 20, 40, 60)] * 3, c, 0, rows, masks, 0, 0, 4)
    with pytest.raises(ValueError):
        E.carry_fill_rungs_host(gens, c, 0, rows, masks[0], 0, 0, 4)


# ---------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------

def test_ladder_plan_regions_are_aligned_in_order_and_end_where_the_next_begins():
    counts, n_rungs, lanes, max_leaves = [3, 274, 0, 15], [3, 1, 8, 2], 65, 300
    off, total, stride = E.carry_ladder_plan_host(counts, n_rungs, lanes, max_leaves)
    n, cols = len(counts), 8 * lanes
    assert len(off) == E.CARRY_SHARED + n * E.CARRY_JOB_REGIONS
    assert all(int(o) % 256 == 0 for o in off) and total % 256 == 0

    def up(b):
        return (b + 255) // 256 * 256
    descs, jobs, first, out = (int(o) for o in off[:4])
    per = np.asarray(off[4:], dtype=np.uint64).reshape(n, 4).astype(object)
    order = [descs, jobs, first] + [int(per[g][k]) for g in range(n) for k in range(3)] + [out] + \
        [int(per[g][3]) for g in range(n)] + [total]
    assert order == sorted(order) and order[0] == 0
    # every region ends where the next begins: its bytes rounded up to 256
    assert first - jobs == up(n * 48) and int(per[0][0]) - first == up(n * 8)
    for g, (k, r) in enumerate(zip(counts, n_rungs)):
        assert int(per[g][1]) - int(per[g][0]) == up((k + 31) // 32 * 4 * r)
        assert int(per[g][2]) - int(per[g][1]) == up(k * 32)
        nxt = int(per[g + 1][0]) if g + 1 < n else out
        assert nxt - int(per[g][2]) == up(k * 24)               # sizeof(mg_leafgen)
    assert int(per[0][3]) - out == up(n * (16 + max_leaves * 32))
    want = up(274 * 8 * cols * 4)
    assert stride * 4 == want
    assert [int(per[g][3]) for g in range(n)] == [int(per[0][3]) + g * want for g in range(n)]
    assert total == int(per[0][3]) + n * want
    # one rung each: the regions of mg_carry_batch's plan but for the rung words of the output
    a = E.carry_ladder_plan_host(counts, [1] * n, lanes, max_leaves)
    b = E.carry_plan_host(counts, lanes, max_leaves)
    assert a[2] == b[2] and np.array_equal(a[0][:4], b[0][:4])
    assert np.array_equal(np.asarray(a[0][4:]).reshape(n, 4)[:, :3],
                          np.asarray(b[0][4:]).reshape(n, 4)[:, :3])


def test_ladder_plan_refusals():
    E.carry_ladder_plan_host([1], [1], 1, 1)
    E.carry_ladder_plan_host([1] * 256, [8] * 256, 1 << 17, 1)
    for counts, n_rungs, lanes in (([], [], 4), ([1] * 257, [1] * 257, 4), ([1], [1], 0),
                                   ([1], [1], (1 << 20) + 1), ([1], [0], 4), ([1], [9], 4),
                                   ([1, 1], [1, 2], (1 << 19) + 1), ([1], [8], (1 << 17) + 1)):
        with pytest.raises(EngineError):
            E.carry_ladder_plan_host(counts, n_rungs, lanes, 1)
    with pytest.raises(EngineError):                           # beyond 64 bits
        E.carry_ladder_plan_host([0xFFFFFFFF] * 256, [8] * 256, 1 << 17, 1)


# ---------------------------------------------------------------------------
# carry.rungs and carry.compile_eval_ck
# ---------------------------------------------------------------------------

def byte(a, k):
    return N.select(a, N.bv_num(k, 256))


def calldata_group(sym_read=False, fresh=False):
    """(parent nodes, new nodes): the parent fixes calldata bytes 0..3 and a
    var; the child reads byte 4 (and, with ``fresh``, a var of its own).  With
    ``sym_read`` the parent also reads the table at a symbolic key."""
    cd = N.array_var("lcd", 256, 8)
    v, u = N.bv_var("lv", 256), N.bv_var("lu", 256)
    parent = [N.eq(byte(cd, k), N.bv_num(0xA0 + k, 8)) for k in range(4)]
    parent.append(N.bv_cmp("bvult", v, N.bv_num(100, 256)))
    if sym_read:
        parent.append(N.eq(N.select(cd, v), N.bv_num(0xA1, 8)))
    new = [N.eq(byte(cd, 4), N.bv_num(0x77, 8))]
    if fresh:
        new.append(N.bv_cmp("bvult", v, u))
    return parent, new


def witness(n=68, v=1):
    """A parent witness as the ABI presets leave it: ``n`` entries, bytes 0..3
    as the parent fixes them, the rest don't-cares (byte 4 not 0x77)."""
    return Assignment(vars={"lv": v}, arrays={"lcd": ([(k, 0xA0 + k & 0xFF) for k in range(n)], 0)})


def masks_by_leaf(prog, masks):
    return [{(l.kind, l.source, l.entry) for i, l in enumerate(prog.leaves) if bit(m, i)}
            for m in masks]


def test_all_is_pins_and_read_frees_the_cval_leaf_the_parent_never_read():
    parent, new = calldata_group()
    asg = witness()
    prog = CY.compile_eval_ck(parent + new, asg)
    assert prog.table_ckeys["lcd"] == [0, 1, 2, 3, 4]
    rows, masks = CY.rungs(prog, asg, parent, new)
    mask, prows = CY.pins(prog, asg)
    assert np.array_equal(masks[0], mask) and np.array_equal(rows, prows)      # "all"
    assert masks.shape == (3, 1) and masks.dtype == np.uint32
    full = CY.rung_masks(prog, asg, parent, new)[1]
    assert full.shape[0] == len(CY.RUNG_NAMES) == 3 and np.array_equal(full, masks)
    every, read, fresh = masks_by_leaf(prog, masks)
    assert every == {("cval", "lcd", e) for e in range(5)} | {("var", "lv", 0)}
    assert every - read == {("cval", "lcd", 4)}
    assert fresh == {("var", "lv", 0)}                          # the new node names the table
    # the rows hold the carried values whatever the rung frees
    vals = leaf_values(prog, asg)
    for l in range(len(prog.leaves)):
        assert int.from_bytes(rows[l].tobytes(), "little") == vals[l]


def test_new_frees_the_leaves_of_names_the_new_nodes_mention():
    parent, new = calldata_group(fresh=True)
    asg = witness()
    prog = CY.compile_eval_ck(parent + new, asg)
    rows, masks = CY.rungs(prog, asg, parent, new)
    assert masks.shape[0] == 3
    every, read, fresh = masks_by_leaf(prog, masks)
    assert every - read == {("cval", "lcd", 4)}
    assert fresh == set()                                       # lcd and lv both occur in the new nodes
    assert ("var", "lu", 0) not in every                        # never pinned: the witness lacks it
    # a child that mentions the table only: the var stays pinned on "new"
    parent, new = calldata_group()
    prog = CY.compile_eval_ck(parent + new, asg)
    full = CY.rung_masks(prog, asg, parent, new)[1]
    assert masks_by_leaf(prog, full)[2] == {("var", "lv", 0)}


def test_a_table_the_parent_reads_at_a_symbolic_key_frees_nothing():
    parent, new = calldata_group(sym_read=True)
    asg = witness(n=6)
    prog = CY.compile_eval_ck(parent + new, asg)
    assert {l.kind for l in prog.leaves if l.source == "lcd"} >= {"cval", "key", "val"}
    # scan_const_keys lists the table (4 keys x 1 link), so the unread cval is free ...
    rows, masks = CY.rungs(prog, asg, parent, new)
    every, read = masks_by_leaf(prog, masks)[:2]
    assert every - read == {("cval", "lcd", 4)}
    assert {k for k in read if k[0] in ("key", "val", "else")} == \
        {k for k in every if k[0] in ("key", "val", "else")} != set()
    # ... but a parent that reads it at symbolic keys only, or past the link cap, frees nothing
    cd, v = N.array_var("lcd", 256, 8), N.bv_var("lv", 256)
    only_sym = [N.eq(N.select(cd, v), N.bv_num(0xA1, 8))]
    full = CY.rung_masks(prog, asg, only_sym, parent[:4] + new)[1]
    assert np.array_equal(full[0], full[1]) and np.array_equal(full[0], CY.pins(prog, asg)[0])
    assert CY.rungs(prog, asg, only_sym, [])[1].shape[0] == 1
    from mythril_amd import ir
    many = [N.eq(N.select(cd, N.bv_op("bvadd", v, N.bv_num(i, 256))), N.bv_num(1, 8))
            for i in range(ir.CKEY_LINKS // 4 + 1)]
    assert "lcd" not in ir.scan_const_keys(parent[:4] + many)
    full = CY.rung_masks(prog, asg, parent[:4] + many, new)[1]
    assert np.array_equal(full[0], full[1])


def test_identical_masks_collapse_and_the_order_is_kept():
    parent, _ = calldata_group()
    v = N.bv_var("lv", 256)
    new = [N.bv_cmp("bvugt", v, N.bv_num(0, 256))]              # reads nothing new of the table
    asg = witness()
    prog = CY.compile_eval_ck(parent + new, asg)
    full = CY.rung_masks(prog, asg, parent, new)[1]
    assert np.array_equal(full[0], full[1]) and not np.array_equal(full[1], full[2])
    assert CY.distinct(full) == [0, 2]
    rows, masks = CY.rungs(prog, asg, parent, new)
    assert masks.shape[0] == 2 and np.array_equal(masks, full[[0, 2]])
    # nothing to free at all: one rung
    rows, masks = CY.rungs(prog, asg, parent + new, [])
    assert masks.shape[0] == 1
    assert CY.distinct(np.zeros((12, 2), dtype=np.uint32)) == [0]
    assert len(CY.distinct(np.arange(12, dtype=np.uint32).reshape(12, 1))) == CY.MAX_RUNGS == 8


def test_compile_eval_ck_sizes_a_68_entry_witness_read_at_constant_keys_at_the_default():
    parent, new = calldata_group()
    asg = witness(68)
    assert CY.table_sizes(asg) == {"lcd": 68}                   # the plain form: above the cap
    assert CY.table_sizes_ck(parent + new, asg) == {"lcd": CY.DEFAULT_ENTRIES}
    prog = CY.compile_eval_ck(parent + new, asg)
    assert prog.table_sizes["lcd"] == CY.DEFAULT_ENTRIES
    assert [l.kind for l in prog.leaves if l.source == "lcd"] == ["cval"] * 5
    assert prog is CY.compile_eval_ck(parent + new, asg)        # cached, apart from the plain form
    plain = CY.compile_eval(parent + new, Assignment(vars={"lv": 1}))
    assert plain is not prog and not plain.table_ckeys.get("lcd")
    assert len(prog.code) < len(CY.compile_eval(parent + new, asg).code) // 4
    # read at a symbolic key too, the entries at other keys are what leaf_values keeps
    parent, new = calldata_group(sym_read=True)
    assert CY.table_sizes_ck(parent + new, asg) == {"lcd": 63}
    assert CY.table_sizes_ck(parent + new, witness(6)) == {"lcd": CY.DEFAULT_ENTRIES}
    prog = CY.compile_eval_ck(parent + new, asg)
    assert prog.table_sizes["lcd"] == 63
    leaf_values(prog, asg)                                      # fits: no ValueError


def test_the_oracle_agrees_that_the_pinned_rows_satisfy_the_parent():
    for sym_read in (False, True):
        parent, new = calldata_group(sym_read=sym_read)
        asg = witness(6)
        prog = CY.compile_eval_ck(parent, asg)
        rows, masks = CY.rungs(prog, asg, parent, [])
        assert masks.shape[0] == 1 and CY.n_free(prog, masks[0]) == 0
        ok = evalref.run_leaves_soa(evalref.serialize(parent, prog), prog,
                                    np.ascontiguousarray(rows[:, :, None]))
        assert ok.tolist() == [True]
        # and the child's "all" rung fails on them: byte 4 is 0xA4, not 0x77
        child = CY.compile_eval_ck(parent + new, asg)
        rows, masks = CY.rungs(child, asg, parent, new)
        ok = evalref.run_leaves_soa(evalref.serialize(parent + new, child), child,
                                    np.ascontiguousarray(rows[:, :, None]))
        assert ok.tolist() == [False]
        l4 = [i for i, l in enumerate(child.leaves) if (l.kind, l.entry) == ("cval", 4)]
        assert len(l4) == 1 and not bit(masks[1], l4[0])
        rows[l4[0]] = 0
        rows[l4[0], 0] = 0x77                                   # what a free leaf may hold
        ok = evalref.run_leaves_soa(evalref.serialize(parent + new, child), child,
                                    np.ascontiguousarray(rows[:, :, None]))
        assert ok.tolist() == [True]


# ---------------------------------------------------------------------------
# the knob and the gate
# ---------------------------------------------------------------------------

def test_knob_2_selects_the_ladder_and_the_statistics_show_rung_hits_only_when_there_are():
    try:
        M.configure_from_env({"MYTHRIL_GPU_CARRY": "2"})
        assert M.CARRY == "ladder"
        M.configure_from_env({"MYTHRIL_GPU_CARRY": "1"})
        assert M.CARRY is True
    finally:
        M.configure_from_env()
    assert M.CARRY is False
    s = M.SolverStatistics()
    s.carry_attempts, s.carry_hits, s.carry_candidates = 2, 1, 513
    assert repr(s).endswith("GPU carry: exact: 0 attempts: 2 hits: 1 candidates: 513")
    s.carry_rung_hits[1] += 1
    assert repr(s).endswith("candidates: 513 rung hits: 0/1/0")
    s.reset_gpu()
    assert s.carry_rung_hits == [0, 0, 0]


def test_the_ladder_gates_on_the_entries_outside_the_constant_keys(monkeypatch):
    parent, new = calldata_group()
    M.clear_search_memos()
    M.stats.reset_gpu()
    key = M._group_key(parent)
    group = [(M._group_key(parent + new), parent + new)]
    try:
        monkeypatch.setattr(M, "CARRY", True)                   # knob 1: 68 entries, gated
        M._note_hit(key, witness(68))
        assert M._carry_groups(group, eng=None) == {}
        assert (M.stats.carry_gated, M.stats.carry_attempts) == (1, 0)
        monkeypatch.setattr(M, "CARRY", "ladder")               # knob 2: a job with its subset keys
        seen = []

        def fake(eng, items, seed, leafgen, lanes=None, phase=None):
            seen.extend(items)
            return [None] * len(items)
        monkeypatch.setattr(CY, "run_ladder", fake)
        assert M._carry_groups(group, eng=object()) == {}
        assert M.stats.carry_gated == 1 and len(seen) == 1
        nodes, asg, taken = seen[0]
        assert taken == [key] and CY.split_nodes(nodes, taken) == (parent, new)
        # a parent that reads the table at a symbolic key keeps 63 entries: gated under knob 2 too
        p2, n2 = calldata_group(sym_read=True)
        M._note_hit(M._group_key(p2), witness(68))
        assert M._carry_groups([(M._group_key(p2 + n2), p2 + n2)], eng=object()) == {}
        assert M.stats.carry_gated == 2 and len(seen) == 1
    finally:
        M.clear_search_memos()
        M.stats.reset_gpu()

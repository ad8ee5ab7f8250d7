"""The delta carry on the GPU (MYTHRIL_GPU_CARRY=5): delta jobs
through Engine.carry_ladder on both register layouts — first, rung and leaves
against oracle/evalref on the columns of mg_carry_fill_rungs_host — and
get_model with knob 5 (on the process's layout) on a hand-built calldata path,
on the trap, on a group the delta refuses and on the stand-in streams.  Every
model is checked on EVERY constraint of its query by oracle/smtlib_ref."""

import json
import os

import numpy as np
import pytest

import delta_cases as D
import mythril_amd.model as M
from mythril_amd import carry as CY
from mythril_amd import workloads as W
from mythril_amd.assign import Assignment, lookup
from mythril_amd.engine import get_engine
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import Array, symbol_factory
from mythril_amd.smt import node as N
from oracle import smtlib_ref as R

pytestmark = pytest.mark.gpu

BVV = symbol_factory.BitVecVal
FIRST = (1 << 32) + 37                    # above 2^32, no multiple of 64


# ---------------------------------------------------------------------------
# parity: three delta jobs in one batch
# ---------------------------------------------------------------------------

def three_jobs():
    """(nodes, witness, taken) of: a one-root delta with no free leaf that
    holds under the witness; the two-root child that reads byte 4 (0x77) and
    holds only where "read" frees it; one that no rung satisfies — "read" frees
    its byte 4, byte 3 stays what the parent made it."""
    parent, new = D.calldata_group()
    cd, v = N.array_var("dcd", 256, 8), N.bv_var("dv", 256)
    taken = [D.key_of(parent)]
    held = [N.bv_cmp("bvugt", D.byte(cd, 3), N.bv_num(5, 8))]
    two = new + [N.bv_cmp("bvult", v, N.bv_num(200, 256))]
    never = new + [N.eq(D.byte(cd, 3), N.bv_num(0, 8))]
    return [(parent + g, D.witness(), taken) for g in (held, two, never)]


@pytest.mark.parametrize("nreg", (16, 11))
def test_first_rung_and_leaves_of_delta_jobs_equal_the_oracle(nreg):
    eng = get_engine(0, nreg=nreg)
    items = three_jobs()
    made = [CY.delta_job(*it) for it in items]
    assert [len(CY.distinct(l)) for _, _, l in made] == [1, 2, 2]
    assert [CY.n_free(p, l[-1]) for p, _, l in made] == [0, 1, 1]
    ref = D.CpuEngine()
    ref.know(items)
    jobs, loaded = [], []
    for (nodes, asg, taken), (prog, rows, ladder) in zip(items, made):
        new = CY.split_nodes(nodes, taken)[1]
        mine = prog if nreg == 16 else compile_constraints(
            new, solve=False, leaf_pools=True, const_keys=True, nreg=nreg,
            table_sizes=CY.table_sizes_ck(new, asg) or None)
        # the leaf order and the pool are the 16-slot program's
        assert [(l.name, l.width) for l in mine.leaves] == [(l.name, l.width) for l in prog.leaves]
        assert mine.const_values == prog.const_values
        masks = ladder[CY.distinct(ladder)]
        jobs.append(((prog, M.search_leafgen(prog), 0), rows, masks))
        loaded.append((eng.load(mine, M.search_leafgen(mine), prog_seed=0), rows, masks))
    for lanes, first in ((1, 0), (63, FIRST), (256, 0)):
        want = ref.carry_ladder(jobs, D.SEED, first, lanes)
        got = eng.carry_ladder(loaded, D.SEED, first, lanes)
        for g, w in zip(got, want):
            assert g[:2] == w[:2], (lanes, g[:2], w[:2])
            assert (g[2] is None) if w[2] is None else np.array_equal(g[2], w[2])
        assert want[0][:2] == (0, 0) and want[2] == (-1, -1, None)
        if lanes == 256:
            assert want[1][1] == 1 and 256 <= want[1][0] < 512
            merged = CY.merge_delta(items[1][1], made[1][0], got[1][2], loaded[1][2][got[1][1]])
            assert lookup(merged.arrays["dcd"], 4) == 0x77 and D.holds(items[1][0], merged) == []


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------

@pytest.fixture
def knob(monkeypatch):
    """MYTHRIL_GPU_CARRY at a value of choice on fresh memos and statistics."""
    def fresh(value):
        monkeypatch.setattr(M, "CARRY", value)
        M.clear_search_memos()
        M.get_model.cache_clear()
        M._batch_witness.clear()
        M._gpu_missed.clear()
        M.stats.reset_gpu()
    M.time_handler.start_execution(3600)
    yield fresh
    monkeypatch.setattr(M, "CARRY", False)
    M.clear_search_memos()
    M.get_model.cache_clear()
    M.stats.reset_gpu()


def model_of(constraints):
    """get_model's assignment, checked on every constraint by the oracle; None
    where get_model has no model."""
    try:
        a = M.get_model(tuple(constraints), enforce_execution_time=False).assignment
    except (M.SolverUnavailable, M.UnsatError):
        return None
    assert D.holds([c.raw for c in constraints], a) == []
    return a


def nodes_of(constraints):
    (b,) = M.dependence_buckets(M._raw_nodes(constraints))      # one group: nothing splits off
    return b


def search_key(constraints):
    return (tuple(n.id for n in nodes_of(constraints)), ())


BYTE4 = 0x77


def test_knob_5_carries_the_child_on_read_by_compiling_its_one_new_constraint(knob):
    cd = Array("delta_calldata", 256, 8)
    parent = [cd[BVV(k, 256)] == BVV(0xA0 + k, 8) for k in range(4)]
    child = parent + [cd[BVV(4, 256)] == BVV(BYTE4, 8)]
    nodes = nodes_of(child)
    pkey, ckey = D.key_of(M._raw_nodes(parent)), D.key_of(nodes)
    old, new = CY.split_nodes(nodes, [pkey])
    assert len(old) == 4 and len(new) == 1
    s = M.stats
    for value in ("delta", "ladder"):
        knob(value)
        w = model_of(parent)
        tab = w.arrays["delta_calldata"]
        assert [lookup(tab, k) for k in range(4)] == [0xA0, 0xA1, 0xA2, 0xA3]
        assert lookup(tab, 4) != BYTE4                          # a don't-care of the parent
        assert (s.carry_attempts, s.carry_delta_attempts) == (0, 0)
        a = model_of(child)                                     # every constraint, by the oracle
        assert lookup(a.arrays["delta_calldata"], 4) == BYTE4
        assert [lookup(a.arrays["delta_calldata"], k) for k in range(4)] == \
            [0xA0, 0xA1, 0xA2, 0xA3]
        assert (s.carry_attempts, s.carry_hits) == (1, 1)
        assert search_key(child) not in M._SEARCH_CACHE         # no solve-mode compile either way
        prog = M._hit_memo.progs[ckey]
        if value == "delta":
            assert (s.carry_delta_attempts, s.carry_delta_hits) == (1, [0, 1])
            assert s.carry_delta_roots == len(new) == 1 != len(nodes)
            assert s.carry_delta_group_roots == len(nodes) == 5
            assert (s.carry_delta_ineligible, s.carry_rung_hits) == (0, [0, 0, 0])
            assert s.carry_candidates == 1 + CY.CARRY_LANES
            assert prog is CY.compile_eval_ck(new, w, CY.table_sizes_ck(new, w))
            assert len(prog.leaves) == 1
            assert "delta attempts: 1 delta hits: 0/1 ineligible: 0 roots: 1 of 5" in repr(s)
            # the merged witness keeps every entry of the parent's
            assert all(lookup(a.arrays["delta_calldata"], k) == lookup(tab, k)
                       for k, _ in tab[0] if k != 4)
            assert a.arrays["delta_calldata"][1] == tab[1]
        else:
            # knob 2 as before: a hit on "read" of the program of EVERY root
            assert s.carry_rung_hits == [0, 1, 0] and s.carry_delta_attempts == 0
            assert s.carry_delta_roots == 0 and "delta" not in repr(s)
            assert prog is CY.compile_eval_ck(nodes, w)
            assert len(prog.leaves) == 5


def test_the_trap_is_no_delta_hit_and_what_comes_back_holds(knob):
    t = Array("delta_trap", 256, 256)
    x = symbol_factory.BitVecSym("delta_tx", 256)
    parent = [t[x] == BVV(1, 256), t[BVV(3, 256)] == BVV(1, 256)]
    child = parent + [t[BVV(5, 256)] == BVV(2, 256)]
    knob("delta")
    asg = Assignment(vars={"delta_tx": 5}, arrays={"delta_trap": ([(5, 1), (3, 1)], 0)})
    praw = M._raw_nodes(parent)
    assert D.holds(praw, asg) == []
    M._note_hit(D.key_of(praw), asg)
    a = model_of(child)                     # whatever it is, it holds on every node
    s = M.stats
    assert (s.carry_delta_attempts, s.carry_delta_hits, s.carry_delta_ineligible) == (1, [0, 0], 0)
    assert s.carry_hits == 0
    if a is not None:                       # the search's own: x has moved off 5
        assert a.vars["delta_tx"] != 5 and lookup(a.arrays["delta_trap"], 5) == 2


def test_a_group_the_delta_refuses_gets_the_ladders_answer(knob):
    w, x = (symbol_factory.BitVecSym(n, 256) for n in ("delta_w", "delta_x"))
    zero = BVV(0, 256)
    parent = [x < BVV(10, 256), (w & zero) == (x & zero)]
    child = parent + [w > BVV(5, 256)]
    got = {}
    s = M.stats
    for value in ("ladder", "delta"):
        knob(value)
        # true whatever delta_w is: the witness is silent about it
        asg = Assignment(vars={"delta_x": 3})
        assert D.holds(M._raw_nodes(parent), asg) == []
        M._note_hit(D.key_of(M._raw_nodes(parent)), asg)
        got[value] = model_of(child)
        assert got[value] is not None and got[value].vars["delta_x"] == 3
        assert (s.carry_attempts, s.carry_hits, s.carry_rung_hits) == (1, 1, [1, 0, 0])
        assert s.carry_delta_ineligible == (1 if value == "delta" else 0)
        assert (s.carry_delta_attempts, s.carry_delta_roots) == (0, 0)
    assert repr(got["delta"]) == repr(got["ladder"])


# ---------------------------------------------------------------------------
# streams, knob 5 against knob off
# ---------------------------------------------------------------------------

HERE = os.path.dirname(os.path.abspath(__file__))
LABELS = json.load(open(os.path.join(HERE, "golden", "recall_labels.json")))


def run_stream(qs):
    out = []
    for q in qs:
        try:
            out.append(M.get_model(tuple(q), enforce_execution_time=False).assignment)
        except (M.SolverUnavailable, M.UnsatError):
            out.append(None)
    return out


@pytest.mark.parametrize("stream", ("c1", "c4"))
def test_streams_lose_no_model_and_gain_no_wrong_one_under_the_delta(knob, stream):
    qs = W.queries(stream, LABELS["n"])[:64]
    unsat = {r["i"] for r in LABELS["streams"].get(stream, ()) if r["label"] == "unsat"}
    knob(False)
    off = run_stream(qs)
    knob("delta")
    on = run_stream(qs)
    s = M.stats
    print("delta %s: models off %d on %d; exact %d attempts %d hits %d delta %d %s ineligible %d "
          "roots %d of %d rungs %s gated %d" % (
              stream, sum(a is not None for a in off), sum(a is not None for a in on),
              s.carry_exact, s.carry_attempts, s.carry_hits, s.carry_delta_attempts,
              s.carry_delta_hits, s.carry_delta_ineligible, s.carry_delta_roots,
              s.carry_delta_group_roots, s.carry_rung_hits, s.carry_gated))
    for i, (q, a, b) in enumerate(zip(qs, off, on)):
        if a is not None:
            assert b is not None, (stream, i)
        if b is not None:
            assert R.eval_constraints(list(q), R.Assignment(b.vars, b.arrays, b.funcs)) == 1, \
                (stream, i)
            assert i not in unsat, (stream, i)
    assert s.carry_exact > 0 and s.carry_delta_attempts > 0
    assert s.carry_delta_roots < s.carry_delta_group_roots

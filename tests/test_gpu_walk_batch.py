"""Many groups' walks in one launch sequence on the GPU (mg_walk_batch,
csrc/mg_walk_batch.hip): every job of a batch equals
Engine.walk_sum on it alone in every output.  The batch mixes jobs that differ
in leaf count, probe count and tables (tests/sum_cases.py, uf_cases.py,
bound_cases.py, aim_cases.py), so every job but the largest lies at a stride
larger than its own size; on both register layouts, at the lane, walker and
sync shapes of tests/test_gpu_walk_sum.py.  Then: jobs that stop at different
sync points (the freeze), the batch reversed, split by a byte cap, one program
in two jobs, a one-job batch, a root mask past one word (tests/gen_cases.py),
and the refusals of the C ABI."""

import ctypes as C
import functools

import numpy as np
import pytest

import aim_cases as AC
import bound_cases as BC
import gen_cases as GC
import sum_cases as SC
import uf_cases as UC
from mythril_amd import engine as E
from mythril_amd import repair as RP
from mythril_amd.engine import EngineError, default_leafgen, get_engine

pytestmark = pytest.mark.gpu

SHORT = 8
# (lanes, walkers, sync_every) at SHORT rounds, as tests/test_gpu_walk_sum.py
PLAN = ((16, 1, 8), (257, 3, 8), (256, 64, 8), (4096, 1, 1))
MIXED = ("sum", "spend", "opaque", "selector", "hash", "shadow", "window", "bytes")


@functools.lru_cache(maxsize=None)
def job_parts(name, nreg=16):
    """(loaded program, starts(walkers), root count, trees, bounds, ufs, sums,
    seed, reference(walkers, lanes, rounds, sync) or None) of a named job."""
    eng = get_engine(0, nreg=nreg)
    if name in SC.NAMES:
        prog, T = SC.program(name, nreg), SC.trees(name)
        B, U, S = SC.tables(name)
        lp = eng.load(SC.view(name, nreg), default_leafgen(prog), prog_seed=0)
        return (lp, lambda w: SC.starts(name, w), len(SC.case(name)[0]), T, B, U, S, SC.SEED,
                lambda *a: SC.reference(name, *a))
    if name in UC.NAMES:
        prog, T = UC.program(name, nreg), UC.trees(name)
        B, U = UC.tables(name)
        lp = eng.load(UC.view(name, nreg), default_leafgen(prog), prog_seed=0)
        return (lp, lambda w: UC.starts(name, w), len(UC.case(name)[0]), T, B, U,
                RP.no_sums(len(B)), UC.SEED, lambda *a: UC.reference(name, *a))
    if name == "window_plain":                     # `window` with tree tables only: plain moves
        lp, st, n_roots, T = job_parts("window", nreg)[:4]
        return (lp, st, n_roots, T, RP.bounds_of_aims(RP.no_aims(), n_roots, T.n_atoms),
                RP.no_ufs(), RP.no_sums(0), BC.SEED, None)
    if name in BC.NAMES:
        prog, T, B = BC.program(name, nreg), BC.trees(name), BC.bounds(name)
        lp = eng.load(prog, default_leafgen(prog), prog_seed=0)
        return (lp, lambda w: BC.starts(name, w), len(BC.case(name)[0]), T, B, RP.no_ufs(),
                RP.no_sums(len(B)), BC.SEED, None)
    prog, T = AC.program(name, nreg), AC.trees(name)
    B = RP.bounds_of_aims(AC.aims(name), len(T.roots), T.n_atoms)
    lp = eng.load(prog, default_leafgen(prog), prog_seed=0)
    return (lp, lambda w: AC.starts(name, w), len(T.roots), T, B, RP.no_ufs(),
            RP.no_sums(len(B)), AC.SEED, None)


def job(name, walkers, nreg=16, seed=None, starts=None):
    lp, st, n_roots, T, B, U, S, sd, _ = job_parts(name, nreg)
    return (lp, st(walkers) if starts is None else starts, n_roots, T, B, U, S,
            sd if seed is None else seed)


def single(eng, j, lanes, rounds, sync=8):
    lp, starts, n_roots, T, B, U, S, seed = j
    return eng.walk_sum(lp, starts, n_roots, T, B, U, S, seed, lanes, rounds, sync)


def same(got, want):
    assert np.array_equal(got.leaves, want.leaves)
    assert np.array_equal(got.nfail, want.nfail) and np.array_equal(got.cost, want.cost)
    assert got.winner == want.winner and got.rounds == want.rounds
    assert np.array_equal(got.trace, want.trace)


@pytest.mark.parametrize("nreg", (16, 11))
def test_mixed_batch_equals_the_single_walks(nreg):
    eng = get_engine(0, nreg=nreg)
    shapes = {(len(job_parts(n, nreg)[0].program.leaves), job_parts(n, nreg)[0].program.n_probes)
              for n in MIXED}
    assert len({s[0] for s in shapes}) > 1 and len({s[1] for s in shapes}) > 1
    for lanes, walkers, sync in PLAN:
        jobs = [job(n, walkers, nreg) for n in MIXED]
        got = eng.walk_batch(jobs, lanes, SHORT, sync)
        assert len(got) == len(MIXED)
        for name, j, g in zip(MIXED, jobs, got):
            assert g.trace.shape == (walkers, SHORT, 2), name
            same(g, single(eng, j, lanes, SHORT, sync))
            ref = job_parts(name, nreg)[8]
            if ref is not None:                                    # walk_ref through the oracle
                same(g, ref(walkers, lanes, SHORT, sync))
        assert got[0].kernel_ms > 0


# `window` under its own table closes in round 1 (bound_cases.FIRST_ZERO), as
# every job of MIXED does: all eight stop at the first sync.  So the batch of
# the freeze test is MIXED and two jobs that go on: `wide` of aim_cases, whose
# first model comes in round 11 (aim_cases.FIRST_ZERO), and `window` without
# its aims, which has only the plain moves.
LONG = MIXED + ("wide", "window_plain")


@functools.lru_cache(maxsize=None)
def long_batch():
    """The batch LONG at 4096 lanes, 1 walker, 32 rounds, sync 8: (jobs, the
    batch's results, the single walks')."""
    eng = get_engine(0)
    jobs = [job(n, 1) for n in LONG]
    return jobs, eng.walk_batch(jobs, 4096, 32, 8), [single(eng, j, 4096, 32) for j in jobs]


def test_jobs_freeze_where_their_own_walks_stop():
    jobs, got, want = long_batch()
    for g, w in zip(got, want):
        same(g, w)
    rounds = dict(zip(LONG, (g.rounds for g in got)))
    print("rounds", rounds)
    assert all(rounds[n] == 8 for n in MIXED)                      # the first sync
    assert AC.FIRST_ZERO["wide"] == 11 and rounds["wide"] == 16    # the second
    assert len(set(rounds.values())) > 1
    for name, g in zip(LONG, got):
        assert not g.trace[:, g.rounds:].any(), name               # nothing past the stop
        assert g.trace[:, :min(g.rounds, 8), 0].any(), name          # and rounds before it
        if g.rounds < 32:
            assert g.nfail.min() == 0, name


def test_order_split_and_a_program_twice():
    eng = get_engine(0)
    jobs, got, _ = long_batch()
    for g, w in zip(eng.walk_batch(jobs[::-1], 4096, 32, 8), got[::-1]):
        same(g, w)
    # a byte cap that forces sub-batches of one or two jobs
    shapes = [E._pack_walk_job(j)["shape"] for j in jobs]
    plan = lambda ss: E.walk_batch_plan_host(ss, 1, 4096, 32)[1]
    two = max(plan(shapes[i:i + 2]) for i in range(len(shapes) - 1))
    one = max(plan([s]) for s in shapes)
    for cap in (two, one):
        parts = E.split_walk_jobs(shapes, 1, 4096, 32, cap)
        print("cap", cap, "parts", parts)
        assert len(parts) > 1 and (cap == two or any(hi - lo == 1 for lo, hi in parts))
        for g, w in zip(eng.walk_batch(jobs, 4096, 32, 8, max_bytes=cap), got):
            same(g, w)
    with pytest.raises(EngineError, match="walk_batch: job 0 alone"):
        eng.walk_batch(jobs, 4096, 32, 8, max_bytes=plan(shapes[:1]) - 1)
    # one loaded program in two jobs, other seeds and starts
    rng = np.random.default_rng(0x6261)
    st = SC.starts("spend", 2).copy()
    st[1] ^= rng.integers(0, 1 << 32, size=st[1].shape, dtype=np.uint32) & np.uint32(0xFF)
    twice = [job("spend", 2), job("spend", 2, seed=SC.SEED + 1, starts=st), job("sum", 2)]
    assert twice[0][0] is twice[1][0]
    res = eng.walk_batch(twice, 257, SHORT, 8)
    for j, g in zip(twice, res):
        same(g, single(eng, j, 257, SHORT))
    assert not np.array_equal(res[0].trace, res[1].trace)


def test_a_one_job_batch_is_the_single_walk():
    eng = get_engine(0)
    for name in ("opaque", "bytes"):
        for lanes, walkers, sync in PLAN:
            j = job(name, walkers)
            (got,) = eng.walk_batch([j], lanes, SHORT, sync)
            same(got, single(eng, j, lanes, SHORT, sync))


@pytest.mark.parametrize("nreg", (16, 11))
def test_a_root_mask_past_one_word(nreg):
    """`rules` of tests/gen_cases.py: 33 roots, a second root-mask word, and
    36 atoms, a second atom-mask word; tree tables only, beside a job of
    another shape on either side."""
    name = "rules"
    assert GC.COUNTS[name][0] > 32
    eng = get_engine(0, nreg=nreg)
    prog, T = GC.program(name, nreg), GC.trees(name)
    lp = eng.load(prog, default_leafgen(prog), prog_seed=0)
    cs = GC.case(name)
    n_roots = len(cs[0] if isinstance(cs, tuple) else cs)
    empty = (RP.bounds_of_aims(RP.no_aims(), n_roots, T.n_atoms), RP.no_ufs(), RP.no_sums(0))
    for lanes, walkers in ((65, 3), (1000, 2)):
        j = (lp, GC.starts(name, walkers), n_roots, T) + empty + (GC.SEED,)
        jobs = [job("spend", walkers, nreg), j, job("bytes", walkers, nreg)]
        got = eng.walk_batch(jobs, lanes, GC.ROUNDS, 8)
        for q, g in zip(jobs, got):
            same(g, single(eng, q, lanes, GC.ROUNDS))
        same(got[1], eng.walk_tree(lp, GC.starts(name, walkers), n_roots, T, GC.SEED, lanes,
                                   GC.ROUNDS))


def test_refusals_launch_nothing_and_leave_the_context_usable():
    import dataclasses
    eng = get_engine(0)
    jobs = [job(n, 2) for n in ("sum", "spend", "hash", "bytes")]
    good = eng.walk_batch(jobs, 256, SHORT, 8)
    ms = eng.last_kernel_ms()
    assert ms > 0

    def with_job(k, **kw):
        lp, starts, n_roots, T, B, U, S, seed = jobs[k]
        d = dict(lp=lp, starts=starts, n_roots=n_roots, trees=T, bounds=B, ufs=U, sums=S, seed=seed)
        d.update(kw)
        out = list(jobs)
        out[k] = (d["lp"], d["starts"], d["n_roots"], d["trees"], d["bounds"], d["ufs"], d["sums"],
                  d["seed"]) + ((d["mask_probe0"],) if "mask_probe0" in d else ())
        return out
    S1 = jobs[1][6]
    lin = np.array(S1.lin, dtype=np.uint32, copy=True)
    lin[0] = RP.SUM_NEG
    other = get_engine(0, nreg=11)
    foreign = job_parts("spend", 11)[0]
    assert foreign.handle != jobs[1][0].handle and other is not eng
    shared = [dict(jobs=[job(n, 65) for n in ("sum", "spend")]), dict(lanes=0),
              dict(lanes=(1 << 20) + 1), dict(max_rounds=0), dict(max_rounds=(1 << 16) + 1)]
    for kw in shared:
        args = dict(jobs=jobs, lanes=256, max_rounds=SHORT, sync_every=8)
        args.update(kw)
        with pytest.raises(EngineError, match=r"\(-1\): walk_batch: "):
            eng.walk_batch(**args)
        assert eng.last_kernel_ms() == ms, kw
    per_job = [(1, dict(sums=dataclasses.replace(S1, lin=lin))),               # a bad lin word
               (1, dict(sums=dataclasses.replace(S1, n_srows=RP.SUM_MAX_ROWS + 1))),
               (2, dict(ufs=dataclasses.replace(jobs[2][5], n_urows=RP.UF_MAX_ROWS + 1))),
               (3, dict(n_roots=0)), (0, dict(mask_probe0=1 << 20)),
               (2, dict(n_roots=1025)),
               (1, dict(lp=foreign))]                                          # another context
    for k, kw in per_job:
        with pytest.raises(EngineError, match=r"\(-1\): walk_batch: job %d: " % k):
            eng.walk_batch(with_job(k, **kw), 256, SHORT, 8)
        assert eng.last_kernel_ms() == ms, (k, kw)
    # a total above max_bytes: the message gives the bytes needed
    need = E.walk_batch_plan_host([E._pack_walk_job(j)["shape"] for j in jobs], 2, 256, SHORT)[1]
    packed = [E._pack_walk_job(j) for j in jobs]
    # the raw ABI: job counts, null pointers, the byte cap
    arr = (E.WalkJob * len(jobs))()
    keep = []
    for i, q in enumerate(packed):
        n_leaves = q["shape"].n_leaves
        bufs = (np.zeros((2, n_leaves, 8), np.uint32), np.zeros(2, np.uint32),
                np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros((2, SHORT, 2), np.uint32))
        keep.append(bufs)
        j = arr[i]
        j.prog = q["lp"].handle
        for f in ("starts", "roots", "atoms", "code", "entries", "pieces", "fixed", "lin", "slots",
                  "funcs", "cands", "ukeys"):
            setattr(j, f, q[f].ctypes.data if q[f].size else None)
        j.out_leaves, j.out_nfail, j.out_cost = (b.ctypes.data for b in bufs[:3])
        j.out_rounds, j.out_winner, j.trace = (bufs[3].ctypes.data, bufs[3].ctypes.data + 4,
                                               bufs[4].ctypes.data)
        j.seed = q["seed"]
        for f in E._WALK_COUNTS:
            setattr(j, f, getattr(q["shape"], f))
    call = lambda a, n, cap=0: eng.lib.mg_walk_batch(eng._ctx, a, n, 2, 256, SHORT, 8, cap)
    err = lambda: eng.lib.mg_last_error(eng._ctx)
    assert call(arr, 0) == -1 and err().startswith(b"walk_batch: 0 jobs")
    assert call(arr, E.WALK_BATCH_MAX_JOBS + 1) == -1 and err().startswith(b"walk_batch: 257 jobs")
    assert call(None, 4) == -1 and err().startswith(b"walk_batch: null")
    assert call(arr, 4, need - 1) == -1
    assert err().startswith(b"walk_batch: %d bytes needed" % need)
    for f in ("prog", "starts", "roots", "out_leaves", "out_nfail", "out_cost", "out_rounds",
              "out_winner"):
        old = getattr(arr[2], f)
        setattr(arr[2], f, None)
        assert call(arr, 4) == -1 and err().startswith(b"walk_batch: job 2: null"), f
        setattr(arr[2], f, old)
    old = arr[1].entries
    arr[1].entries = None                                       # a table with a count
    assert call(arr, 4) == -1 and err().startswith(b"walk_batch: job 1: ")
    arr[1].entries = old
    assert eng.last_kernel_ms() == ms
    # and the same array goes through, within exactly the bytes of the plan
    assert call(arr, 4, need) == 0
    for g, bufs in zip(good, keep):
        assert np.array_equal(bufs[0], g.leaves) and np.array_equal(bufs[1], g.nfail)
        assert np.array_equal(bufs[2], g.cost) and tuple(bufs[3]) == (g.rounds, g.winner)
        assert np.array_equal(bufs[4], g.trace)
    for g, w in zip(eng.walk_batch(jobs, 256, SHORT, 8), good):
        same(g, w)


# ---------------------------------------------------------------------------
# repair_groups and batch_is_possible
# ---------------------------------------------------------------------------

def oracle_values(constraints, a):
    from oracle import smtlib_ref as R
    return R.evaluate(list(constraints), R.Assignment(a.vars, a.arrays, a.funcs))


def equal(a, b, path="result"):
    """a and b field by field: arrays by value, dataclasses and objects by
    their fields, DAG nodes by identity; kernel_ms is not compared."""
    import dataclasses
    assert type(a) is type(b), path
    if isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    elif isinstance(a, dict):
        assert list(a) == list(b), path
        for k in a:
            equal(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            equal(x, y, "%s[%d]" % (path, i))
    elif dataclasses.is_dataclass(a):
        for f in dataclasses.fields(a):
            if f.name != "kernel_ms":
                equal(getattr(a, f.name), getattr(b, f.name), "%s.%s" % (path, f.name))
    elif hasattr(a, "id") and hasattr(a, "op"):
        assert a is b, path                                   # hash-consed nodes
    elif hasattr(a, "__dict__"):
        equal(vars(a), vars(b), path)
    else:
        assert a == b, path


def test_repair_groups_equals_repair_group_per_group():
    from mythril_amd import census as CS
    from mythril_amd.smt import node as N
    x = N.bv_var("wb_refuted_x", 256)
    groups = [list(SC.case(n)[0]) for n in SC.STUCK]
    groups.insert(1, [N.bool_val(True)])                                  # ground true
    groups.append([N.eq(x, N.bv_num(1, 256)), N.eq(x, N.bv_num(2, 256))])  # refuted on the host
    kw = dict(form="eval", max_rounds=8, scored="sum", walkers=1)
    calls = []
    eng = get_engine(0)
    batch = type(eng).walk_batch
    try:
        type(eng).walk_batch = lambda self, jobs, *a, **k: (calls.append(len(jobs)),
                                                             batch(self, jobs, *a, **k))[1]
        got = RP.repair_groups(groups, **kw)
    finally:
        type(eng).walk_batch = batch
    want = [RP.repair_group(g, **kw) for g in groups]
    assert calls == [3]                                       # one batch, the three walks
    assert [g["status"] for g in got] == [RP.REPAIRED, CS.GROUND_TRUE, RP.REPAIRED, RP.REPAIRED,
                                          CS.REFUTED]
    for i, (g, w) in enumerate(zip(got, want)):
        equal(g, w, "group %d" % i)
        if g["status"] == RP.REPAIRED:
            assert g["scoring"] == "sum" and g["repair"].rounds <= 8
            assert all(oracle_values(groups[i], g["assignment"]))
    assert RP.repair_groups([], **kw) == []


SPENDS = 3


def spend_query(prefix):
    """The `spend` query of tests/test_gpu_walk_sum.py (SPENDS spends over one
    t), over symbols of its own."""
    import walk_cases as WK
    from mythril_amd.smt import Concat, Extract, Not, ULE, ULT, symbol_factory
    val = symbol_factory.BitVecVal
    sym = lambda s, w=256: symbol_factory.BitVecSym(prefix + "_" + s, w)
    p, q = sym("p"), sym("q")
    rng = np.random.default_rng(0x7371)
    p0 = WK._guarded(int.from_bytes(rng.bytes(32), "little"), (64, 128))
    q0 = WK._guarded(int.from_bytes(rng.bytes(32), "little"), (64, 128)) ^ (
        0x1111 << 64 | 0x1111 << 128)
    K = (p0 ^ q0) - 1
    cons = [p == val(p0, 256), q == val(q0, 256)]
    for i in range(SPENDS):
        bal, v = sym("bal%d" % i), sym("v%d" % i)
        s = Concat(Extract(127, 0, bal), Extract(255, 128, bal)) - v
        cons += [ULT(val(K, 256), s), ULE(s, (p ^ q) + val(3, 256))]
        cons += [Not(Extract(lo + 15, lo, x) == val(k, 16)) for x in (bal, v) for lo in (64, 128)
                 for k in (0, 0xFFFF)]
    return tuple(cons)


@pytest.fixture
def model_state():
    import mythril_amd.model as M
    get_engine(0)                                  # not on the query's budget
    M.get_model.cache_clear()
    M.clear_search_memos()
    M.time_handler.start_execution(3600)
    M.stats.reset_gpu()
    yield M
    M.configure_from_env({})
    M.SEARCH_BUDGET_MS = 200
    M.clear_search_memos()
    M.get_model.cache_clear()
    M.stats.reset_gpu()


def test_batch_is_possible_repairs_the_missed_groups_in_one_batch(model_state):
    M = model_state
    M.configure_from_env({"MYTHRIL_GPU_REPAIR": "7", "MYTHRIL_GPU_REPAIR_BATCH": "1",
                          "MYTHRIL_GPU_BUDGET_MS": "5000"})
    assert M.REPAIR_BATCH and M.REPAIR_SCORED == "sum"
    sets = [spend_query("wbq%d" % i) for i in range(4)]
    assert M.batch_is_possible(sets, enforce_execution_time=False) == [True] * 4
    assert M.stats.repair_batches == 1
    assert (M.stats.repair_attempts, M.stats.repair_hits) == (4, 4)
    assert M.stats.gpu_hits == 4 and not M._group_miss
    assert "batches: 1" in M.stats.gpu_report()
    for cons in sets:
        m = M.get_model(cons, enforce_execution_time=False)         # the cached answer
        assert all(oracle_values([c.raw for c in cons], m.assignment))


def test_without_the_knob_batch_is_possible_repairs_nothing(model_state):
    M = model_state
    M.configure_from_env({"MYTHRIL_GPU_REPAIR": "7", "MYTHRIL_GPU_BUDGET_MS": "5000"})
    assert not M.REPAIR_BATCH
    sets = [spend_query("wbn%d" % i) for i in range(2)]
    try:                                     # (z3 absent: nothing decides a miss)
        M.batch_is_possible(sets, enforce_execution_time=False)
    except M.SolverUnavailable:
        pass
    assert M.stats.repair_batches == 0
    assert "batches" not in M.stats.gpu_report()

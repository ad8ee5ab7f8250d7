"""The census of a pin ladder on the GPU (mg_carry_census,
csrc/mg_carry_census.hip): every rung's census, the start
columns and their rows against the oracle on the specified columns on both
register layouts, start 0 against mg_carry_ladder, the surplus columns of a job
with fewer rungs than its batch, the refusals of the C ABI, and get_model with
MYTHRIL_GPU_CARRY=3 on a hand-built path and on the stand-in streams."""

import ctypes as C
import functools

import numpy as np
import pytest

import census_cases as K
import gen_cases as G
import mythril_amd.model as M
import test_gpu_carry_ladder as TL
from mythril_amd import carry as CY
from mythril_amd import census as CS
from mythril_amd import engine as E
from mythril_amd import repair as RP
from mythril_amd import workloads as W
from mythril_amd.assign import lookup
from mythril_amd.engine import Gen, default_leafgen, get_engine
from mythril_amd.smt import Array, Concat, symbol_factory
from oracle import evalref
from oracle import smtlib_ref as R

pytestmark = pytest.mark.gpu

SEED = TL.SEED
FIRST = TL.FIRST                          # above 2^32, no multiple of 64
L5, L33, L257 = ("ladder", 5), ("ladder", 33), ("ladder", 257)
# case -> (prog_seed, thresholds), as the ladder's test has them
CASES = dict(TL.CASES)
CASES.update({L33: (3, "default"), L257: (5, "default")})
WALKERS = (1, 4, 64)


def built(case, nreg=16):
    if isinstance(case, tuple):
        return K.masked_program(case, nreg)
    return G.case(case), G.program(case, nreg, "mask")


def leafgen(case, prog):
    return M.search_leafgen(prog) if CASES[case][1] == "search" else default_leafgen(prog)


@functools.lru_cache(maxsize=None)
def loaded(case, nreg=16):
    prog = built(case, nreg)[1]
    return get_engine(0, nreg=nreg).load(prog, leafgen(case, prog), prog_seed=CASES[case][0])


def test_the_shapes_are_those_the_kernels_branch_on():
    shapes = {c: (len(built(c)[1].leaves), (len(built(c)[0]) + 31) // 32, built(c)[1].n_probes)
              for c in (L5, L33, L257)}
    assert shapes == {L5: (3, 1, 1), L33: (3, 2, 1), L257: (3, 9, 2)}
    assert len(built("flats")[1].leaves) == 274 and len(built("rules")[1].leaves) == 15


@functools.lru_cache(maxsize=None)
def serialized(case):
    cs, prog = built(case)
    return evalref.serialize(cs, prog)


def spec(case, masks, rows, first, lanes, top):
    """(soa, censuses) of a job in a batch of ``top`` rungs: the columns
    mg_carry_fill_rungs_host specifies and, per rung of the job, the census of
    the oracle's verdicts on that rung's columns."""
    prog = built(case)[1]
    soa = E.carry_fill_rungs_host(leafgen(case, prog), prog.consts, CASES[case][0], rows, masks,
                                  SEED, first, lanes, cols=top * lanes)
    bits = evalref.run_leaves_soa(serialized(case), prog, soa, per_root=True)
    assert bits.shape == (top * lanes, len(built(case)[0]))
    return soa, [CS.reduce_bits(bits[r * lanes:(r + 1) * lanes], r * lanes)
                 for r in range(masks.shape[0])]


def rung1_first(lanes):
    """A first index above 2^32 at which the second of ``three_outcomes`` (y
    broken, only x pinned on rung 1) has a model among rung 1's ``lanes``
    candidates: from the oracle's verdicts on the candidates from FIRST on."""
    _, masks, rows = TL.three_outcomes()[1]
    prog = built(L5)[1]
    soa = E.carry_fill_rungs_host(leafgen(L5, prog), prog.consts, CASES[L5][0], rows, masks[1:],
                                  SEED, FIRST, 256)
    hit = np.flatnonzero(evalref.run_leaves_soa(serialized(L5), prog, soa))
    assert hit.size
    return FIRST + max(0, int(hit[0]) - (lanes - 1))


def batches():
    """Two batches of jobs ``(case, masks, rows)`` mixing 3, 1 and 2 rungs."""
    o = TL.three_outcomes()
    first = [o[0], (L5, o[2][1][:1], o[2][2]), o[1]]
    second = [(c,) + TL.random_rungs(c, 71 + k, n, share)
              for k, (c, n, share) in enumerate(((L257, 3, 0.4), ("flats", 1, 0.5),
                                                 ("rules", 2, 0.3), (L33, 2, 0.4)))]
    return first, second


def args_of(jobs, nreg=16):
    return [(loaded(c, nreg), r, m, len(built(c)[0])) for c, m, r in jobs]


# ---------------------------------------------------------------------------
# parity with the specification
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", (1, 63, 65, 256))
@pytest.mark.parametrize("nreg", (16, 11))
def test_censuses_starts_and_rows_equal_the_specification(nreg, lanes):
    eng = get_engine(0, nreg=nreg)
    first = rung1_first(lanes)
    assert first > 1 << 32
    seen = set()
    for jobs in batches():
        top = max(m.shape[0] for _, m, _ in jobs)
        assert top == 3 and {1, 2, 3} <= {m.shape[0] for _, m, _ in jobs}
        want = [spec(c, m, r, first, lanes, top) for c, m, r in jobs]
        for walkers in WALKERS:
            res = eng.carry_census(args_of(jobs, nreg), SEED, first, lanes, walkers)
            assert eng.last_kernel_ms() > 0
            for (case, m, _), (soa, cs), (got_cs, col, nfail, rows) in zip(jobs, want, res):
                assert len(got_cs) == m.shape[0]
                for r, (a, b) in enumerate(zip(got_cs, cs)):
                    assert a == b, (case, lanes, r, a.as_dict(), b.as_dict())
                    assert (a.first_index, a.n_cand) == (r * lanes, lanes)
                want_col, want_nfail = CY.starts_ref(cs, walkers)
                assert col.tolist() == want_col.tolist(), (case, lanes, walkers)
                assert nfail.tolist() == want_nfail.tolist(), (case, lanes, walkers)
                assert rows.shape == (walkers, soa.shape[0], 8)
                for w in range(walkers):
                    assert np.array_equal(rows[w], soa[:, :, int(col[w])]), (case, lanes, w)
                # the situations, from the oracle's censuses alone
                n = m.shape[0] + sum(int(((c.sole_index >= 0) &
                                          (c.sole_index != c.best_index)).sum()) for c in cs)
                seen.add("longer" if n > walkers else "padding" if n < walkers else "exact")
                if want_nfail[0] == 0 and want_col[0] // lanes == 1:
                    seen.add("rung 1")
    assert {"longer", "padding", "rung 1"} <= seen


def test_zero_rows_past_a_programs_leaves_through_the_raw_abi():
    eng = get_engine(0)
    (jobs, _), lanes, walkers = batches(), 65, 4
    keep = [(np.ascontiguousarray(r), np.ascontiguousarray(m)) for _, m, r in jobs]
    arr = (E.CarryCensusJob * 3)()
    for i, (r, m) in enumerate(keep):
        lad = arr[i].ladder
        lad.prog, lad.pin_rows, lad.pin_masks, lad.n_rungs = (loaded(L5).handle, E._ptr(r),
                                                              E._ptr(m), m.shape[0])
        arr[i].n_roots, arr[i].mask_probe0 = 5, 0
    counts = np.full((3, 3, 5 * 7 + 2), 0xAB, dtype=np.uint64)
    col = np.full((3, walkers), 7, dtype=np.int64)
    nfail = np.full((3, walkers), 7, dtype=np.uint32)
    rows = np.full((3, walkers, 5, 8), 0xAB, dtype=np.uint32)
    g = Gen(SEED, FIRST)
    assert eng.lib.mg_carry_census(eng._ctx, arr, 3, C.byref(g), lanes, walkers, 7, 5,
                                   E._ptr(counts), E._ptr(col), E._ptr(nfail), E._ptr(rows),
                                   None) == 0
    want = [spec(c, m, r, FIRST, lanes, 3) for c, m, r in jobs]
    for i, (soa, cs) in enumerate(want):
        n = len(cs)
        for r in range(3):
            block = counts[i, r]
            if r < n:
                assert CS.unpack_block(block[:27], 5, r * lanes, lanes) == cs[r]
                assert not block[27:].any()
            else:
                assert not block.any()                    # a rung the job does not have
        assert not rows[i, :, 3:].any()                   # past the program's 3 leaves
        for w in range(walkers):
            assert np.array_equal(rows[i, w, :3], soa[:, :, int(col[i, w])])


# ---------------------------------------------------------------------------
# start 0 is the ladder's answer
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", (65, 256))
def test_start_0_is_what_carry_ladder_returns(lanes):
    eng = get_engine(0)
    first = rung1_first(lanes)
    hits = 0
    for jobs in batches():
        res = eng.carry_census(args_of(jobs), SEED, first, lanes, 4)
        old = eng.carry_ladder([(loaded(c), r, m) for c, m, r in jobs], SEED, first, lanes)
        for (_, col, nfail, rows), (f0, rung0, leaves0) in zip(res, old):
            if nfail[0] == 0:
                assert (int(col[0]), int(col[0]) // lanes) == (f0, rung0)
                assert np.array_equal(rows[0], leaves0)
                hits += 1
            else:
                assert (f0, rung0, leaves0) == (-1, -1, None)
    assert hits >= 2


# ---------------------------------------------------------------------------
# the surplus columns are evaluated and not counted
# ---------------------------------------------------------------------------

def test_a_job_alone_and_in_a_batch_of_more_rungs_gives_the_same_censuses():
    eng = get_engine(0)
    for lanes in (63, 256):
        for jobs in batches():
            mixed = eng.carry_census(args_of(jobs), SEED, FIRST, lanes, 4)
            for job, got in zip(jobs, mixed):
                if job[1].shape[0] == max(m.shape[0] for _, m, _ in jobs):
                    continue
                (alone,) = eng.carry_census(args_of([job]), SEED, FIRST, lanes, 4)
                assert alone[0] == got[0]
                assert alone[1].tolist() == got[1].tolist()
                assert alone[2].tolist() == got[2].tolist()
                assert np.array_equal(alone[3], got[3])


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def test_the_job_cap_and_the_refusals():
    eng = get_engine(0)
    jobs, _ = batches()
    args = args_of(jobs)
    res = eng.carry_census(args, SEED, FIRST, 64, 4)
    assert eng.carry_census([], SEED, FIRST, 64, 4) == []
    many = (args * 86)[:257]
    got = eng.carry_census(many, SEED, FIRST, 64, 4)      # 257 jobs: split at 256
    assert len(got) == 257
    for k, g in enumerate(got):
        assert g[0] == res[k % 3][0] and g[1].tolist() == res[k % 3][1].tolist()
    ms = eng.last_kernel_ms()
    with pytest.raises(ValueError):
        eng.carry_census([(args[0][0], args[0][1], args[0][2][0], 5)], SEED, FIRST, 64, 4)

    def raw(n_jobs, lanes, max_leaves, walkers=4, max_roots=5, handles=None, rows=True,
            masks=True, null=None, n_rungs=None, n_roots=None, probe0=None):
        arr = (E.CarryCensusJob * max(1, n_jobs))()
        for i in range(n_jobs):
            lp, r, m, k = many[i]
            lad = arr[i].ladder
            lad.prog = handles[i] if handles else lp.handle
            lad.pin_rows = E._ptr(r) if rows else None
            lad.pin_masks = E._ptr(m) if masks else None
            lad.n_rungs = m.shape[0] if n_rungs is None else n_rungs[i]
            arr[i].n_roots = k if n_roots is None else n_roots[i]
            arr[i].mask_probe0 = 0 if probe0 is None else probe0[i]
        n, w = max(1, n_jobs), max(1, min(walkers, 64))
        bufs = {"counts": np.zeros((n, 8, 5 * max(1, min(max_roots, 1024)) + 2), dtype=np.uint64),
                "col": np.zeros((n, w), dtype=np.int64), "nfail": np.zeros((n, w), dtype=np.uint32),
                "rows": np.zeros((n, w, max(1, min(max_leaves, 8)), 8), dtype=np.uint32)}
        ptr = {k: (None if k == null else E._ptr(v)) for k, v in bufs.items()}
        g = Gen(SEED, FIRST)
        rc = eng.lib.mg_carry_census(eng._ctx, None if null == "jobs" else arr, n_jobs,
                                     None if null == "gen" else C.byref(g), lanes, walkers,
                                     max_roots, max_leaves, ptr["counts"], ptr["col"],
                                     ptr["nfail"], ptr["rows"], None)
        return rc, eng.lib.mg_last_error(eng._ctx)

    # whatever mg_carry_ladder refuses
    assert raw(257, 64, 3) == (-1, b"carry_census: 257 jobs outside 1..256")
    assert raw(0, 64, 3) == (-1, b"carry_census: 0 jobs outside 1..256")
    assert raw(2, 0, 3) == (-1, b"carry_census: 0 lanes outside 1..1048576")
    assert raw(2, (1 << 20) + 1, 3) == (-1, b"carry_census: 1048577 lanes outside 1..1048576")
    for null in ("jobs", "gen", "counts", "col", "nfail", "rows"):
        assert raw(2, 64, 3, null=null) == (-1, b"carry_census: null argument")
    assert raw(2, 64, 3, rows=False) == (-1, b"carry_census: job 0: null pin rows or pin masks")
    assert raw(2, 64, 3, masks=False) == (-1, b"carry_census: job 0: null pin rows or pin masks")
    assert raw(2, 64, 3, handles=[many[0][0].handle, None]) == \
        (-1, b"carry_census: job 1: null program")
    other = loaded(L5, 11)                              # a program of the 11-slot context
    assert raw(2, 64, 3, handles=[many[0][0].handle, other.handle]) == \
        (-1, b"carry_census: job 1: a program of another context")
    assert raw(2, 64, 2) == (-1, b"carry_census: job 0: 3 leaves above max_leaves 2")
    rc, why = raw(2, 64, (1 << 20) + 1)
    assert rc == -1 and why.startswith(b"carry_census: max_leaves")
    assert raw(2, 64, 3, n_rungs=[3, 0]) == (-1, b"carry_census: job 1: 0 rungs outside 1..8")
    assert raw(2, 64, 3, n_rungs=[9, 1]) == (-1, b"carry_census: job 0: 9 rungs outside 1..8")
    assert raw(3, (1 << 20) // 3 + 1, 3) == \
        (-1, b"carry_census: 3 rungs of 349526 lanes above 1048576 columns")
    # its own: walkers, n_roots, max_roots, the mask probes
    assert raw(2, 64, 3, walkers=0) == (-1, b"carry_census: 0 walkers outside 1..64")
    assert raw(2, 64, 3, walkers=65) == (-1, b"carry_census: 65 walkers outside 1..64")
    assert raw(2, 64, 3, n_roots=[5, 0]) == (-1, b"carry_census: job 1: n_roots 0 outside 1..1024")
    assert raw(2, 64, 3, max_roots=2000, n_roots=[1025, 5]) == \
        (-1, b"carry_census: job 0: n_roots 1025 outside 1..1024")
    assert raw(2, 64, 3, max_roots=4) == (-1, b"carry_census: job 0: n_roots 5 above max_roots 4")
    assert raw(2, 64, 3, probe0=[0, 1]) == \
        (-1, b"carry_census: job 1: mask probes 1..1 outside the program's 1 probes")
    assert raw(2, 64, 3, max_roots=300, n_roots=[5, 257]) == \
        (-1, b"carry_census: job 1: mask probes 0..1 outside the program's 1 probes")
    # 256 jobs of 274 leaves at 2^17 lanes: above the buffer the call may take
    flats = loaded("flats")
    m, r = TL.random_rungs("flats", 1, 8, 0.5)
    with pytest.raises(E.EngineError, match="carry_census: .* bytes needed for 256 jobs"):
        eng.carry_census([(flats, r, m, len(built("flats")[0]))] * 256, SEED, 0, 1 << 17, 4)
    assert eng.last_kernel_ms() == ms                   # nothing was launched
    again = eng.carry_census(args, SEED, FIRST, 64, 4)  # and the context is still usable
    for a, b in zip(res, again):
        assert a[0] == b[0] and np.array_equal(a[3], b[3])


# ---------------------------------------------------------------------------
# end to end: a child no rung can meet, repaired by the walk from start 0
# ---------------------------------------------------------------------------

BVV = symbol_factory.BitVecVal
LOW = 0x34567890ABCDEF_0FEDCBA098765432_1122334455667788_99AABBCCDDEEFF00       # 248 bits


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


def sum_path():
    """(parent, child): the §3.19 test's parent — calldata bytes 0..3 fixed —
    and a child that adds ``a + b == calldata[0] . LOW`` on two fresh 256-bit
    symbols: one value of 2^256 for the sum, so no rung meets it by chance, and
    one aimed move away from any start that has the bytes right."""
    cd = Array("walk_calldata", 256, 8)
    a, b = (symbol_factory.BitVecSym("walk_" + s, 256) for s in "ab")
    parent = [cd[BVV(k, 256)] == BVV(0xA0 + k, 8) for k in range(4)]
    return parent, parent + [a + b == Concat(cd[BVV(0, 256)], BVV(LOW, 248))]


def oracle_ok(constraints, a):
    return R.eval_constraints([c.raw for c in constraints],
                              R.Assignment(a.vars, a.arrays, a.funcs)) == 1


def test_knob_3_walks_a_child_that_misses_every_rung_to_a_model(knob):
    """What the miss report must say follows from the pins, not from a run: on
    rung "all" every calldata byte is pinned to the parent's witness, so the
    four parent constraints hold on every column and the added one is the only
    blocker, satisfied nowhere.  On rung "new" the bytes are free as well (the
    added constraint mentions the table, and that rung frees every leaf of a
    name the new nodes mention), so the parent's constraints fail there too and
    may rank above it; the added one — one value of 2^256 for the sum — still
    fails on some column and is listed."""
    parent, child = sum_path()
    (nodes,) = M.dependence_buckets(M._raw_nodes(child))
    taken = [M._group_key(M._raw_nodes(parent))]
    old, new = CY.split_nodes(nodes, taken)
    assert len(old) == 4 and len(new) == 1
    added = nodes.index(new[0])
    s = M.stats
    for value in ("ladder", "walk"):
        knob(value)
        m = M.get_model(tuple(parent), enforce_execution_time=False)
        w = m.assignment
        assert oracle_ok(parent, w)
        assert (s.carry_attempts, s.carry_walk_attempts) == (0, 0)
        # the oracle generator: no column of any rung is a model within CARRY_LANES
        prog = CY.compile_census_ck(nodes, w, CS.mask_probes(nodes))
        rows, masks = CY.rungs(prog, w, old, new)
        assert masks.shape[0] >= 2
        soa = E.carry_fill_rungs_host(M.search_leafgen(prog), prog.consts, 0, rows, masks,
                                      M.SEARCH_SEED, 0, CY.CARRY_LANES)
        bits = evalref.run_leaves_soa(evalref.serialize(nodes, prog), prog, soa, per_root=True)
        assert not bits.all(axis=1).any()
        if value == "ladder":
            try:                                  # tried, missed; the search decides the rest
                M.get_model(tuple(child), enforce_execution_time=False)
            except (M.SolverUnavailable, M.UnsatError):
                pass
            assert (s.carry_attempts, s.carry_hits) == (1, 0)
            assert (s.carry_walk_attempts, s.carry_walk_hits) == (0, 0)
            assert "walks:" not in repr(s)
            continue
        launches = s.launches
        a = M.get_model(tuple(child), enforce_execution_time=False).assignment
        assert oracle_ok(child, a)
        assert (s.carry_attempts, s.carry_hits) == (1, 0)
        assert (s.carry_walk_attempts, s.carry_walk_hits) == (1, 1)
        assert "walks: 1 walk hits: 1" in repr(s)
        assert s.launches >= launches + 3 + 4 + 3         # ladder, census, one round at least
        tab = a.arrays["walk_calldata"]
        assert [lookup(tab, k) for k in range(4)] == [0xA0, 0xA1, 0xA2, 0xA3]
        assert (a.vars["walk_a"] + a.vars["walk_b"]) % (1 << 256) == (0xA0 << 248) | LOW
        # the same through repair_carried, with its report
        (g,) = RP.repair_carried([(nodes, w, taken)], CY.CARRY_LANES, 4, max_rounds=16)
        assert g["status"] == RP.REPAIRED and g["scoring"] == "sum"
        assert oracle_ok(child, g["assignment"])
        assert g["start"] == {"col": 0, "rung": 0, "nfail": 1} and g["starts"][0] == 0
        assert [CY.RUNG_NAMES[r] for r in g["rungs"]] == [r["rung"] for r in g["miss_report"]]
        for r, c in zip(g["miss_report"], g["census"]):
            c.check()
            roots = [x["root"] for x in r["blockers"]]
            assert added in roots and int(c.pass_[added]) < c.n_cand, r
            assert r["blockers"][roots.index(added)]["constraint"] == repr(new[0])
        assert [x["root"] for x in g["miss_report"][0]["blockers"]] == [added]
        assert g["miss_report"][0]["blockers"][0]["pass"] == 0


# ---------------------------------------------------------------------------
# streams, knob 3 against knob off
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("stream", ("c4", "c5"))
def test_streams_lose_no_model_and_gain_no_wrong_one_under_the_walk(knob, stream):
    qs = W.queries(stream, TL.LABELS["n"])[:64]
    unsat = {r["i"] for r in TL.LABELS["streams"].get(stream, ()) if r["label"] == "unsat"}
    knob(False)
    off = TL.run_stream(qs)
    knob("walk")
    on = TL.run_stream(qs)
    s = M.stats
    print("walk %s: models off %d on %d; exact %d attempts %d hits %d rungs %s walks %d walk hits "
          "%d" % (stream, sum(a is not None for a in off), sum(a is not None for a in on),
                  s.carry_exact, s.carry_attempts, s.carry_hits, s.carry_rung_hits,
                  s.carry_walk_attempts, s.carry_walk_hits))
    for i, (q, a, b) in enumerate(zip(qs, off, on)):
        if a is not None:
            assert b is not None, (stream, i)
        if b is not None:
            assert R.eval_constraints(list(q), R.Assignment(b.vars, b.arrays, b.funcs)) == 1, \
                (stream, i)
            assert i not in unsat, (stream, i)
    assert s.carry_exact > 0
    assert s.carry_walk_hits <= s.carry_walk_attempts <= s.carry_attempts - s.carry_hits

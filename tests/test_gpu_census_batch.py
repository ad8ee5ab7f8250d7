"""Many programs' verdict censuses in one launch sequence on the GPU
(mg_census_batch, csrc/mg_census_batch.hip): every job of a
batch equals Engine.census on it alone and the oracle's recount
(tests/census_cases.py) in every field, on both register layouts; chunks and
merged halves; the job cap and a grid that strides; order; mg_batch_witness
against Engine.witness; explain_groups and repair_groups against their
per-group forms; and the refusals of the C ABI."""

import ctypes as C
import functools

import numpy as np
import pytest

import census_cases as K
from mythril_amd import census as CS
from mythril_amd import engine as E
from mythril_amd import repair as RP
from mythril_amd.engine import EngineError, Gen, default_leafgen, get_engine

pytestmark = pytest.mark.gpu

LADDERS = tuple(("ladder", R) for R in K.RS)
MIXED = LADDERS + (("c2", 7), ("c4", 16))
FIRST20, N20 = 1 << 20, 4096


@functools.lru_cache(maxsize=None)
def loaded(key, nreg=16):
    """(the case's masked eval-form program loaded with the oracle's generator
    parameters on the engine of the layout, its root count)."""
    cs, prog = K.masked_program(key, nreg)
    ref = K.masked_program(key)[1]               # the oracle's pool is this program's
    assert prog.const_values == ref.const_values and len(prog.leaves) == len(ref.leaves)
    eng = get_engine(0, nreg=nreg)
    return eng.load(prog, default_leafgen(prog), prog_seed=K.PROG_SEED), len(cs)


def jobs_of(keys, nreg=16):
    return [loaded(k, nreg) + (0,) for k in keys]


@functools.lru_cache(maxsize=None)
def single(key, first, n, nreg=16):
    lp, r = loaded(key, nreg)
    return get_engine(0, nreg=nreg).census(lp, K.SEED, first, n, r)


@functools.lru_cache(maxsize=None)
def mixed_batch(nreg=16):
    return get_engine(0, nreg=nreg).census_batch(jobs_of(MIXED, nreg), K.SEED, FIRST20, N20)


@pytest.mark.parametrize("nreg", (16, 11))
def test_mixed_batch_equals_the_single_census_and_the_oracle(nreg):
    eng = get_engine(0, nreg=nreg)
    got = mixed_batch(nreg)
    assert len(got) == len(MIXED)
    for key, g in zip(MIXED, got):
        want = CS.reduce_bits(K.oracle_bits(key, FIRST20, N20), FIRST20)
        assert g.as_dict() == want.as_dict(), (key, nreg)
        assert g == single(key, FIRST20, N20, nreg), (key, nreg)
        g.check()
    assert got[0].kernel_ms > 0
    # the batch really mixes: leaf counts, probe regions of 1 and 2 mask probes,
    # satisfied and unsatisfied jobs (the C4 unit has no satisfying lane)
    progs = [loaded(k, nreg)[0].program for k in MIXED]
    assert len({len(p.leaves) for p in progs}) > 1
    assert {p.n_probes for p in progs} >= {1, 2}
    assert any(g.best_nfail == 0 for g in got) and any(g.best_nfail > 0 for g in got)
    assert got[MIXED.index(("c4", 16))].n_sat == 0
    # an index above 2^32, tails that are no multiple of 64 or 256
    for n in (1, 63, 64, 65, 1000):
        res = eng.census_batch(jobs_of(LADDERS, nreg), K.SEED, K.FIRST, n)
        for key, g in zip(LADDERS, res):
            want = CS.reduce_bits(K.oracle_bits(key)[:n], K.FIRST)
            assert g.as_dict() == want.as_dict(), (key, nreg, n)
            assert g == single(key, K.FIRST, n, nreg)


def test_chunks_and_merged_halves_give_the_same_census():
    eng = get_engine(0)
    keys = (("ladder", 33), ("ladder", 257))
    jobs = jobs_of(keys)
    whole = eng.census_batch(jobs, K.SEED, K.FIRST, K.N_CAND)
    for key, w in zip(keys, whole):
        assert w == CS.reduce_bits(K.oracle_bits(key), K.FIRST)
    assert eng.census_batch(jobs, K.SEED, K.FIRST, K.N_CAND, chunk=256) == whole
    assert eng.census_batch(jobs, K.SEED, K.FIRST, K.N_CAND, chunk=512) == whole
    a = eng.census_batch(jobs, K.SEED, K.FIRST, 448)
    b = eng.census_batch(jobs, K.SEED, K.FIRST + 448, K.N_CAND - 448, chunk=256)
    assert [x.merge(y) for x, y in zip(a, b)] == whole


def test_the_cap_and_the_strided_grid():
    eng = get_engine(0)
    keys = LADDERS * 32
    assert len(keys) == E.CENSUS_BATCH_MAX_JOBS == 256
    jobs = jobs_of(keys)
    assert jobs[0][0] is jobs[8][0]                          # one program in many jobs
    tiles = N20 // 256
    assert 0 < E.census_batch_blocks_host(256, N20) < tiles  # tiles are grid-strided
    assert E.split_census_jobs([E.CensusShape(lp.program.n_probes, r, m)
                                for lp, r, m in jobs]) == [(0, 256)]
    got = eng.census_batch(jobs, K.SEED, FIRST20, N20, chunk=N20)
    assert len(got) == 256
    for key, g in zip(keys, got):
        assert g == single(key, FIRST20, N20), key
    # 257 jobs: Engine.census_batch splits, the raw ABI refuses
    more = jobs + jobs[3:4]
    res = eng.census_batch(more, K.SEED, FIRST20, N20, chunk=N20)
    assert len(res) == 257 and res[:256] == got and res[256] == got[3]
    ms = eng.last_kernel_ms()
    arr = (E.CensusJob * 257)()
    for i, (lp, r, m) in enumerate(more):
        arr[i].prog, arr[i].n_roots, arr[i].mask_probe0 = lp.handle, r, m
    out = raw_outputs(257, 257)
    g = Gen(K.SEED, FIRST20)
    assert eng.lib.mg_census_batch(eng._ctx, arr, 257, C.byref(g), N20, N20, 257, *out) == -1
    assert eng.lib.mg_last_error(eng._ctx).startswith(b"census_batch: 257 jobs outside 1..256")
    assert eng.last_kernel_ms() == ms


def test_a_one_job_batch_and_a_reversed_batch():
    eng = get_engine(0)
    for key in (("ladder", 3), ("ladder", 257), ("c4", 16)):
        (got,) = eng.census_batch(jobs_of([key]), K.SEED, FIRST20, N20)
        assert got == single(key, FIRST20, N20)
    back = eng.census_batch(jobs_of(MIXED[::-1]), K.SEED, FIRST20, N20)
    assert back == mixed_batch()[::-1]
    assert eng.census_batch([], K.SEED, FIRST20, N20) == []


# ---------------------------------------------------------------------------
# mg_batch_witness
# ---------------------------------------------------------------------------

def test_batch_witness_equals_the_single_witness():
    eng = get_engine(0)
    pairs = []
    for key, c in zip(MIXED, mixed_batch()):
        lp = loaded(key)[0]
        pairs.append((lp, c.best_index))
        pairs += [(lp, int(i)) for i in c.sole_index if i >= 0]
    assert len(pairs) > len(MIXED) and len({id(lp) for lp, _ in pairs}) == len(MIXED)
    got = eng.batch_witness(pairs, K.SEED)
    assert len(got) == len(pairs)
    for (lp, i), (leaves, probes) in zip(pairs, got):
        wl, wp = eng.witness(lp, K.SEED, i)
        assert leaves.shape == wl.shape and probes.shape == wp.shape
        assert leaves.tobytes() == np.ascontiguousarray(wl).tobytes()
        assert probes.tobytes() == np.ascontiguousarray(wp).tobytes()
    # without the probes, one program three times, and index -1
    lp = loaded(("ladder", 33))[0]
    three = [(lp, K.FIRST), (lp, -1), (lp, K.FIRST + 999), (loaded(("c2", 7))[0], -1), (lp, 5)]
    res = eng.batch_witness(three, K.SEED, want_probes=False)
    for (p, i), (leaves, probes) in zip(three, res):
        assert probes is None
        if i < 0:
            assert leaves.shape == (len(p.program.leaves), 8) and not leaves.any()
        else:
            assert np.array_equal(leaves, eng.witness(p, K.SEED, i)[0])
    zero = eng.batch_witness(three, K.SEED)[1]
    assert not zero[0].any() and not zero[1].any() and zero[1].shape == (lp.program.n_probes, 8)
    assert eng.batch_witness([], K.SEED) == []


def test_search_form_batch_finds_the_search_programs_first_witness():
    """The C1 groups of tests/test_gpu_census.py's search-form test, their
    views in one batch: first_sat per group is Engine.search's index on the
    full masked program, and the batched witness is the search's."""
    import mythril_amd.model as M
    from mythril_amd import workloads as W
    eng = get_engine(0)
    jobs, fulls, want = [], [], []
    for q in W.queries("c1", 64)[:4]:
        for group in M.dependence_buckets(q):
            if M._ground_value(M._compile_search_uncached(group)) is not None:
                continue
            full = M._compile_search_uncached(group, CS.mask_probes(group))
            assert full.n_user_probes == 1
            gens = M.search_leafgen(full)
            fulls.append(eng.load(full, gens, prog_seed=0))
            want.append(eng.search(fulls[-1], M.SEARCH_SEED, 1 << 14))
            jobs.append((eng.load(CS.census_view(full, 1), gens, prog_seed=0), len(group), 0))
    assert len(jobs) > 1
    got = eng.census_batch(jobs, M.SEARCH_SEED, 0, 1 << 14)
    for c, (idx, _) in zip(got, want):
        c.check()
        assert c.first_sat == idx and (c.best_nfail == 0) == (idx >= 0)
    assert any(idx >= 0 for idx, _ in want)
    wit = eng.batch_witness([(lp, c.first_sat) for lp, c in zip(fulls, got)], M.SEARCH_SEED)
    for (leaves, _), (idx, w) in zip(wit, want):
        if idx >= 0:
            assert np.array_equal(leaves, w)
        else:
            assert not leaves.any()


# ---------------------------------------------------------------------------
# explain_groups and repair_groups
# ---------------------------------------------------------------------------

class single_calls_raise:
    """Engine.census and Engine.witness raise; census_batch and batch_witness
    are counted."""

    def __enter__(self):
        self.cls = type(get_engine(0))
        self.saved = {n: getattr(self.cls, n) for n in ("census", "witness", "census_batch",
                                                        "batch_witness")}
        self.calls = {"census_batch": [], "batch_witness": []}

        def refuse(name):
            def f(*a, **k):
                raise AssertionError("Engine.%s called under a batched driver" % name)
            return f

        def count(name):
            inner = self.saved[name]

            def f(eng, items, *a, **k):
                self.calls[name].append(len(items))
                return inner(eng, items, *a, **k)
            return f
        self.cls.census, self.cls.witness = refuse("census"), refuse("witness")
        self.cls.census_batch, self.cls.batch_witness = count("census_batch"), count("batch_witness")
        return self

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(self.cls, n, f)


def test_explain_groups_equals_explain_group_per_group():
    import json
    import os
    import mythril_amd.model as M
    from mythril_amd import workloads as W
    from test_gpu_walk_batch import equal
    labels = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                         "recall_labels.json")))
    qs = W.queries("c4", labels["n"])
    q = qs[16]
    # the groups of query 16 (one of them is launched), then those of its
    # neighbours, so that the batch holds several programs
    groups = [list(b) for b in M.dependence_buckets(q)]
    own = len(groups)
    groups += [list(b) for k in (15, 17, 18) for b in M.dependence_buckets(qs[k])]
    kw = dict(n_cand=1 << 14, form="search")
    want = [CS.explain_group(g, **kw) for g in groups]
    launched = [w for w in want if "census" in w]
    assert any("census" in w and w["census"].n_sat == 0 for w in want[:own])
    print("c4 groups", len(groups), "launched", len(launched))
    assert len(launched) > 1
    with single_calls_raise() as patched:
        got = CS.explain_groups(groups, **kw)
    assert patched.calls == {"census_batch": [len(launched)], "batch_witness": [len(launched)]}
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        equal(g, w, "group %d" % i)
    # and explain is built on it: the same entries, positions mapped back
    with single_calls_raise():
        rep = CS.explain(q, **kw)
    assert [g["status"] for g in rep["groups"]] == [w["status"] for w in want[:own]]
    for g, w in zip(rep["groups"], want):
        assert g.get("census") == w.get("census")
    assert CS.explain_groups([], **kw) == []


def test_repair_groups_prepares_in_batches():
    import sum_cases as SC
    from mythril_amd.smt import node as N
    from test_gpu_walk_batch import equal
    x = N.bv_var("cb_refuted_x", 256)
    groups = [list(SC.case(n)[0]) for n in SC.STUCK]
    groups.insert(1, [N.bool_val(True)])                                  # ground true
    groups.append([N.eq(x, N.bv_num(1, 256)), N.eq(x, N.bv_num(2, 256))])  # refuted on the host
    kw = dict(form="eval", max_rounds=8, scored="sum", walkers=3)
    with single_calls_raise() as patched:
        got = RP.repair_groups(groups, **kw)
    walks = len(SC.STUCK)
    assert patched.calls == {"census_batch": [walks], "batch_witness": [3 * walks]}
    want = [RP.repair_group(g, **kw) for g in groups]
    assert [g["status"] for g in got] == [w["status"] for w in want]
    assert sum(g["status"] == RP.REPAIRED for g in got) == walks
    for i, (g, w) in enumerate(zip(got, want)):
        equal(g, w, "group %d" % i)


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def raw_outputs(n, width):
    """The seven output arrays of mg_census_batch as pointers (kept alive by
    the list's owner)."""
    arrays = [np.zeros((n, width), np.uint64) for _ in range(3)] + \
        [np.zeros((n, width), np.int64), np.zeros((n, width + 1), np.uint64),
         np.zeros(n, np.uint32), np.zeros(n, np.int64)]
    out = [a.ctypes.data_as(C.c_void_p) for a in arrays]
    raw_outputs.keep = arrays
    return out


def test_refusals_launch_nothing_and_leave_the_context_usable():
    eng = get_engine(0)
    keys = (("ladder", 33), ("ladder", 257), ("ladder", 3), ("c2", 7))
    jobs = jobs_of(keys)
    good = eng.census_batch(jobs, K.SEED, K.FIRST, 256)
    assert good == [single(k, K.FIRST, 256) for k in keys]
    ms = eng.last_kernel_ms()
    assert ms > 0
    refused = r"\(-1\): .*census_batch"
    # the shared arguments of mg_census
    for kw in (dict(chunk=100), dict(chunk=384 + 64), dict(first_index=K.FIRST + 1),
               dict(first_index=K.FIRST + 32), dict(n_cand=1 << 53),
               dict(first_index=(1 << 63) - 64, n_cand=128)):
        args = dict(jobs=jobs, seed=K.SEED, first_index=K.FIRST, n_cand=256)
        args.update(kw)
        with pytest.raises(EngineError, match=refused + ": (chunk|first_index|[0-9]+ candidates)"):
            eng.census_batch(**args)
        assert eng.last_kernel_ms() == ms, kw
    # the buffer: a chunk past the byte cap names the bytes
    need = 4 * 2 * 32 * (1 << 24)
    with pytest.raises(EngineError, match=refused + ": %d bytes needed" % need):
        eng.census_batch(jobs, K.SEED, K.FIRST, 256, chunk=1 << 24)
    assert eng.last_kernel_ms() == ms
    # per job: what mg_census refuses for it, and a program of another context
    other = get_engine(0, nreg=11)
    foreign = loaded(("ladder", 33), 11)[0]
    assert other is not eng and foreign.handle != jobs[0][0].handle
    per_job = [(0, (jobs[0][0], 0, 0)), (1, (jobs[1][0], 1025, 0)), (2, (jobs[2][0], 257, 0)),
               (3, (jobs[3][0], jobs[3][1], 1)), (1, (jobs[1][0], 257, 1 << 20)),
               (2, (foreign, 33, 0))]
    for k, j in per_job:
        bad = list(jobs)
        bad[k] = j
        with pytest.raises(EngineError, match=refused + ": job %d: " % k):
            eng.census_batch(bad, K.SEED, K.FIRST, 256)
        assert eng.last_kernel_ms() == ms, (k, j[1:])
    # the raw ABI: job counts, null pointers, rows narrower than a job
    arr = (E.CensusJob * 4)()
    for i, (lp, r, m) in enumerate(jobs):
        arr[i].prog, arr[i].n_roots, arr[i].mask_probe0 = lp.handle, r, m
    out = raw_outputs(4, 257)
    g = Gen(K.SEED, K.FIRST)
    call = lambda a, n, o, gen=C.byref(g), width=257: eng.lib.mg_census_batch(
        eng._ctx, a, n, gen, 256, 0, width, *o)
    err = lambda: eng.lib.mg_last_error(eng._ctx)
    assert call(arr, 0, out) == -1 and err().startswith(b"census_batch: 0 jobs")
    assert call(None, 4, out) == -1 and err().startswith(b"census_batch: null")
    assert call(arr, 4, out, gen=None) == -1 and err().startswith(b"census_batch: null")
    for k in range(7):
        o = list(out)
        o[k] = None
        assert call(arr, 4, o) == -1 and err().startswith(b"census_batch: null"), k
    old = arr[2].prog
    arr[2].prog = None
    assert call(arr, 4, out) == -1 and err().startswith(b"census_batch: job 2: null")
    arr[2].prog = old
    assert call(arr, 4, out, width=256) == -1
    assert err().startswith(b"census_batch: job 1: n_roots 257 above max_roots 256")
    assert eng.last_kernel_ms() == ms
    # batch_witness refuses before it launches, too
    lp = jobs[0][0]
    with pytest.raises(EngineError, match=r"\(-1\): batch_witness: pair 1: index -2"):
        eng.batch_witness([(lp, 0), (lp, -2)], K.SEED)
    with pytest.raises(EngineError, match=r"\(-1\): batch_witness: pair 0: a program of another"):
        eng.batch_witness([(foreign, 0)], K.SEED)
    assert eng.last_kernel_ms() == ms
    # an empty range: empty censuses, no launch
    empty = eng.census_batch(jobs, K.SEED, K.FIRST, 0)
    for (lp, r, _), c in zip(jobs, empty):
        assert c == CS.reduce_bits(np.zeros((0, r), dtype=bool), K.FIRST)
        assert (c.best_nfail, c.best_index) == (r + 1, -1)
    assert eng.last_kernel_ms() == ms
    # the same array goes through the raw entry, and the next valid call succeeds
    assert call(arr, 4, out) == 0
    a = raw_outputs.keep
    for i, c in enumerate(good):
        r = c.n_roots
        assert np.array_equal(a[0][i, :r], c.pass_) and not a[0][i, r:].any()
        assert np.array_equal(a[3][i, :r], c.sole_index) and (a[3][i, r:] == -1).all()
        assert np.array_equal(a[4][i, :r + 1], c.nfail_hist)
        assert (int(a[5][i]), int(a[6][i])) == (c.best_nfail, c.best_index)
    assert eng.census_batch(jobs, K.SEED, K.FIRST, 256) == good

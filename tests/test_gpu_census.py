"""The verdict census on the GPU (mg_census, csrc/mg_census.hip; DESIGN.md
§3.8): Engine.census against reduce_masks of the oracle's per-constraint bits
(oracle/evalref.c, its own generator) in every field, on both register
layouts; chunking and merging; the refusals of the C ABI; a search-form hit;
and the miss report of C4 query 16."""

import ctypes as C

import numpy as np
import pytest

import census_cases as K
from mythril_amd import census as CS
from mythril_amd.engine import EngineError, Gen, default_leafgen, get_engine

pytestmark = pytest.mark.gpu


def loaded(key, nreg=16):
    """(engine of the layout, the case's masked eval-form program loaded with
    the oracle's generator parameters, its root count)."""
    cs, prog = K.masked_program(key, nreg)
    ref = K.masked_program(key)[1]               # the oracle's pool is this program's
    assert prog.const_values == ref.const_values and len(prog.leaves) == len(ref.leaves)
    eng = get_engine(0, nreg=nreg)
    return eng, eng.load(prog, default_leafgen(prog), prog_seed=K.PROG_SEED), len(cs)


@pytest.mark.parametrize("nreg", (16, 11))
@pytest.mark.parametrize("R", K.RS)
def test_census_equals_the_oracle_on_the_ladder(R, nreg):
    """1000 candidates from 2^33 + 64 (a tail that is no multiple of 64,
    indices above 2^32), and ranges of 1, 63, 64 and 65 candidates."""
    key = ("ladder", R)
    eng, lp, n_roots = loaded(key, nreg)
    assert n_roots == R and eng.nreg == nreg
    bits = K.oracle_bits(key)
    for n in (K.N_CAND, 1, 63, 64, 65):
        got = eng.census(lp, K.SEED, K.FIRST, n, R)
        want = CS.reduce_bits(bits[:n], K.FIRST)
        assert got.as_dict() == want.as_dict(), (R, nreg, n)
        got.check()
    assert got.kernel_ms > 0


@pytest.mark.parametrize("R", (33, 257))
def test_chunks_and_merged_halves_give_the_same_census(R):
    eng, lp, _ = loaded(("ladder", R))
    whole = eng.census(lp, K.SEED, K.FIRST, K.N_CAND, R)
    assert whole == CS.reduce_bits(K.oracle_bits(("ladder", R)), K.FIRST)
    assert eng.census(lp, K.SEED, K.FIRST, K.N_CAND, R, chunk=256) == whole
    assert eng.census(lp, K.SEED, K.FIRST, K.N_CAND, R, chunk=512) == whole
    a = eng.census(lp, K.SEED, K.FIRST, 448, R)
    b = eng.census(lp, K.SEED, K.FIRST + 448, K.N_CAND - 448, R, chunk=256)
    assert a.merge(b) == whole


@pytest.mark.parametrize("key", (("c2", 7), ("c4", 16)), ids=lambda k: "%s%d" % k)
def test_census_of_bench_units_equals_the_oracle(key):
    eng, lp, n_roots = loaded(key)
    first, n = 1 << 20, 4096
    want = CS.reduce_bits(K.oracle_bits(key, first, n), first)
    assert eng.census(lp, K.SEED, first, n, n_roots) == want
    assert eng.census(lp, K.SEED, first, n, n_roots, chunk=1024) == want


def test_bits_at_or_above_n_roots_are_ignored():
    eng, lp, _ = loaded(("ladder", 33))
    bits = K.oracle_bits(("ladder", 33))
    assert bits[:, 20:].any()
    assert eng.census(lp, K.SEED, K.FIRST, K.N_CAND, 20) == CS.reduce_bits(bits[:, :20], K.FIRST)


def test_search_form_hit_is_the_search_programs_first_witness():
    """A C1 group the search solves: the census of the view finds the index
    Engine.search finds on the full masked program, with no failing root."""
    import mythril_amd.model as M
    from mythril_amd import workloads as W
    eng = get_engine(0)
    hits = 0
    for q in W.queries("c1", 64)[:4]:
        for group in M.dependence_buckets(q):
            if M._ground_value(M._compile_search_uncached(group)) is not None:
                continue
            full = M._compile_search_uncached(group, CS.mask_probes(group))
            assert full.n_user_probes == 1
            gens = M.search_leafgen(full)
            idx, _ = eng.search(eng.load(full, gens, prog_seed=0), M.SEARCH_SEED, 1 << 14)
            c = eng.census(eng.load(CS.census_view(full, 1), gens, prog_seed=0), M.SEARCH_SEED, 0,
                           1 << 14, len(group))
            c.check()
            assert c.first_sat == idx and (c.best_nfail == 0) == (idx >= 0)
            hits += idx >= 0
    assert hits > 0


def test_explain_names_the_blockers_of_c4_query_16():
    import json
    import os
    import mythril_amd.model as M
    from mythril_amd import workloads as W
    from oracle import smtlib_ref as R
    labels = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                         "recall_labels.json")))
    q = W.queries("c4", labels["n"])[16]
    def state():
        return (dict(M._group_miss), {k: list(v) for k, v in M._shape_stats.items()},
                len(M._SEARCH_CACHE or ()), M.stats.gpu_report())
    before = state()
    rep = M.explain_miss(q, n_cand=1 << 16, form="search")
    assert state() == before                 # no memo, gate or statistic moved
    assert sorted(p for g in rep["groups"] for p in g["constraints"]) == list(range(len(q)))
    launched = [g for g in rep["groups"] if g["status"] == CS.CENSUS]
    assert launched and any(g["census"].n_sat == 0 for g in launched)
    for g in launched:
        c = g["census"]
        c.check()
        assert c.n_cand == 1 << 16 and c.n_roots == len(g["constraints"])
        best = g["best"]
        assert (best["index"], best["nfail"]) == (c.best_index, c.best_nfail)
        assert len(best["failing"]) == c.best_nfail
        a = best["assignment"]
        vals = R.evaluate([q[p] for p in g["constraints"]], R.Assignment(a.vars, a.arrays, a.funcs))
        assert best["failing"] == [p for p, v in zip(g["constraints"], vals) if not v]
        if c.n_sat == 0:
            assert best["failing"] and set(best["failing"]) <= set(g["blockers"])
            print("c4 q16 blockers", g["blockers"][:8], "best", best["index"], best["failing"])
    again = M.explain_miss(q, n_cand=1 << 16, form="search")
    for g, h in zip(rep["groups"], again["groups"]):
        assert g["status"] == h["status"] and g.get("census") == h.get("census")
        assert g.get("blockers") == h.get("blockers")
        if "best" in g:
            assert g["best"]["failing"] == h["best"]["failing"]
            assert repr(g["best"]["assignment"]) == repr(h["best"]["assignment"])


def test_refusals_launch_nothing_and_leave_the_context_usable():
    eng, lp, _ = loaded(("ladder", 33))
    good = eng.census(lp, K.SEED, K.FIRST, 256, 33)
    ms = eng.last_kernel_ms()
    assert ms > 0
    bad = [dict(n_roots=0), dict(n_roots=1025), dict(n_roots=257), dict(mask_probe0=1),
           dict(chunk=100), dict(chunk=384 + 64), dict(first_index=K.FIRST + 1),
           dict(first_index=K.FIRST + 32), dict(chunk=1 << 24)]
    for kw in bad:
        args = dict(seed=K.SEED, first_index=K.FIRST, n_cand=256, n_roots=33)
        args.update(kw)
        with pytest.raises(EngineError, match=r"\(-1\): .*census") as e:
            eng.census(lp, **args)
        if kw == dict(chunk=1 << 24):
            assert "census view" in str(e.value)
        assert eng.last_kernel_ms() == ms, kw          # no launch was timed
    # a null pointer
    u = [np.zeros(34, dtype=np.uint64) for _ in range(4)]
    si = np.zeros(33, dtype=np.int64)
    bn, bi = C.c_uint32(), C.c_int64()
    p = [a.ctypes.data_as(C.c_void_p) for a in u[:3]] + [si.ctypes.data_as(C.c_void_p),
                                                        u[3].ctypes.data_as(C.c_void_p)]
    g = Gen(K.SEED, K.FIRST)
    for k in range(5):
        q = list(p)
        q[k] = None
        rc = eng.lib.mg_census(eng._ctx, lp.handle, C.byref(g), 256, 33, 0, 0, *q, C.byref(bn),
                               C.byref(bi))
        assert rc == -1 and b"null" in eng.lib.mg_last_error(eng._ctx)
    assert eng.lib.mg_census(eng._ctx, None, C.byref(g), 256, 33, 0, 0, *p, C.byref(bn),
                             C.byref(bi)) == -1
    assert eng.last_kernel_ms() == ms
    # an empty range: zeros, -1 indices, best_nfail = n_roots + 1, no launch
    empty = eng.census(lp, K.SEED, K.FIRST, 0, 33)
    assert empty == CS.reduce_bits(np.zeros((0, 33), dtype=bool), K.FIRST)
    assert (empty.best_nfail, empty.best_index) == (34, -1) and eng.last_kernel_ms() == ms
    # and the next valid call succeeds
    assert eng.census(lp, K.SEED, K.FIRST, 256, 33) == good

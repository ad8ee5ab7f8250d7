#!/usr/bin/env python3
"""Measurements of the witness carry, knob on
against knob off in one process on the GPU:

* recall -- every labelled stream of tests/golden/recall_labels.json in order
  through ``get_model``: SAT-labelled queries found, UNSAT-labelled queries
  with a model, models the oracle rejects, the carry's counters;
* lanes -- the carry hit rate on extensions of c4 and c5 at 64, 256, 1024 and
  4096 candidates (``carry.CARRY_LANES``), at the default table cap and with
  the cap lifted;
* compile -- with the cap lifted, the dearest eval-form compile of each stream:
  its time, the group's constraints, the carried table sizes, records, leaves;
* kernel -- device time (``Engine.last_kernel_ms``) and wall time of one
  ``Engine.carry_batch`` call at 1, 64 and 256 jobs.

Usage:  python tools/carry_measure.py [out.json]   (progress lines on stdout)
"""

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LANES = (64, 256, 1024, 4096)
NO_CAP = 1 << 30


def fresh(M, on):
    M.CARRY = on
    M.clear_search_memos()
    M.get_model.cache_clear()
    M._batch_witness.clear()
    M._gpu_missed.clear()
    M.stats.reset_gpu()


def stream(M, qs):
    out = []
    for q in qs:
        try:
            out.append(M.get_model(tuple(q), enforce_execution_time=False).assignment)
        except (M.SolverUnavailable, M.UnsatError):
            out.append(None)
    return out


def counters(M):
    s = M.stats
    return {"exact": s.carry_exact, "attempts": s.carry_attempts, "hits": s.carry_hits,
            "table_gated": s.carry_gated, "candidates": s.carry_candidates,
            "launches": s.launches, "launch_calls": s.kernel_calls}


def recall(M, W, R):
    labels = json.load(open(os.path.join(ROOT, "tests", "golden", "recall_labels.json")))
    out, tot = {}, {False: [0, 0], True: [0, 0]}
    for name in sorted(labels["streams"]):
        rows = labels["streams"][name]
        qs = W.queries(name, labels["n"])
        line = {}
        for on in (False, True):
            fresh(M, on)
            t0 = time.perf_counter()
            got = stream(M, qs)
            dt = time.perf_counter() - t0
            sat = [r["i"] for r in rows if r["label"] == "sat"]
            found = [i for i in sat if got[i] is not None]
            line["on" if on else "off"] = dict(counters(M), **{
                "sat_labelled": len(sat), "found": len(found),
                "missed": sorted(set(sat) - set(found)),
                "unsat_with_model": [r["i"] for r in rows
                                     if r["label"] == "unsat" and got[r["i"]] is not None],
                "wrong_models": [i for i, a in enumerate(got) if a is not None and
                                 R.eval_constraints(list(qs[i]), R.Assignment(
                                     a.vars, a.arrays, a.funcs)) != 1],
                "models": sum(a is not None for a in got), "wall_s": round(dt, 3)})
            tot[on][0] += len(found)
            tot[on][1] += len(sat)
        out[name] = line
        print("recall", name, json.dumps(line), flush=True)
    out["total"] = {"off": tot[False], "on": tot[True]}
    print("recall total", out["total"], flush=True)
    return out


def lanes_and_compile(M, W, CY):
    lanes, compiles = {}, {}
    base, cap = CY.CARRY_LANES, CY.MAX_ENTRIES
    orig = CY.compile_eval
    log = []

    def traced(nodes, asg):
        n0 = len(CY._EVAL_CACHE)
        t = time.perf_counter()
        p = orig(nodes, asg)
        if len(CY._EVAL_CACHE) != n0:                    # compiled, not cached
            log.append({"ms": round((time.perf_counter() - t) * 1e3, 2),
                        "constraints": len(nodes), "table_sizes": CY.table_sizes(asg),
                        "records": int(p.n_ins), "leaves": len(p.leaves)})
        return p
    CY.compile_eval = traced
    try:
        for name, n in (("c4", 128), ("c5", 256)):
            qs = W.queries(name, n)
            for entries in (cap, NO_CAP):
                CY.MAX_ENTRIES = entries
                for width in LANES:
                    CY.CARRY_LANES = width
                    fresh(M, True)
                    del log[:]
                    t0 = time.perf_counter()
                    got = stream(M, qs)
                    key = "%s@%d%s" % (name, width, "" if entries == cap else " uncapped")
                    lanes[key] = dict(counters(M), models=sum(a is not None for a in got),
                                      wall_s=round(time.perf_counter() - t0, 3))
                    print("lanes", key, lanes[key], flush=True)
                    if entries == NO_CAP and width == base and log:
                        compiles[name] = {"compiles": len(log),
                                          "total_ms": round(sum(r["ms"] for r in log), 2),
                                          "dearest": max(log, key=lambda r: r["ms"])}
                        print("compile", name, compiles[name], flush=True)
    finally:
        CY.compile_eval, CY.CARRY_LANES, CY.MAX_ENTRIES = orig, base, cap
    return lanes, compiles


def kernel_times(eng):
    """One carry call of a 33-root ladder over three 16-bit symbols, nothing
    pinned."""
    from mythril_amd.engine import default_leafgen
    from mythril_amd.ir import compile_constraints
    from mythril_amd.smt import node as N
    x, y, z = (N.bv_var(s, 16) for s in ("kx", "ky", "kz"))
    cs = [N.bv_cmp("bvult", x, N.bv_num(65535 - k * 1985, 16)) for k in range(31)]
    cs += [N.bv_cmp("bvult", y, N.bv_num(1 << 15, 16)), N.distinct(y, z)]
    prog = compile_constraints(cs)
    lp = eng.load(prog, default_leafgen(prog), prog_seed=3)
    n = len(prog.leaves)
    rows, mask = np.zeros((n, 8), np.uint32), np.zeros((n + 31) // 32, np.uint32)
    out = {}
    for jobs in (1, 64, 256):
        for width in (1, 256, 4096):
            ms, wall = [], []
            for _ in range(12):
                t0 = time.perf_counter()
                eng.carry_batch([(lp, rows, mask)] * jobs, 1, 0, width)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(eng.last_kernel_ms())
            key = "%d jobs x %d lanes" % (jobs, width)
            out[key] = {"kernel_ms_median": float(np.median(ms[2:])),
                        "wall_ms_median": float(np.median(wall[2:]))}
            print("kernel", key, out[key], flush=True)
    return out


def main():
    import mythril_amd.model as M
    from mythril_amd import carry as CY
    from mythril_amd import workloads as W
    from mythril_amd.engine import get_engine
    from oracle import smtlib_ref as R                   # checker only
    M.time_handler.start_execution(36000)
    res = {"recall": recall(M, W, R)}
    res["lanes"], res["compile"] = lanes_and_compile(M, W, CY)
    res["kernel"] = kernel_times(get_engine(0))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

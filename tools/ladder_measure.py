#!/usr/bin/env python3
"""Measurements of the pin ladder, in one
process on the GPU; the counterpart of tools/carry_measure.py, whose helpers it
uses:

* recall -- every labelled stream of tests/golden/recall_labels.json in order
  through ``get_model`` with the knob off and with ``MYTHRIL_GPU_CARRY=2``: SAT-
  labelled queries found, UNSAT-labelled queries with a model, models the
  oracle rejects, the carry's counters and its hits per rung;
* compile -- under knob 2, the eval-form compiles of the c4 (128 queries) and c5
  (256) streams: their number and total time, and the dearest: its time, the
  group's constraints, the table sizes, records and leaves;
* kernel -- device time (``Engine.last_kernel_ms``, median of 10) and wall time
  of one ``Engine.carry_ladder`` call at 1, 64 and 256 jobs x 256 lanes x 1 and 3
  rungs, beside ``Engine.carry_batch`` at the same total columns in the same run.

Usage:  python tools/ladder_measure.py [out.json]   (progress lines on stdout)
"""

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import carry_measure as CM  # noqa: E402


def counters(M):
    return dict(CM.counters(M), rung_hits=list(M.stats.carry_rung_hits))


def recall(M, W, R):
    labels = json.load(open(os.path.join(ROOT, "tests", "golden", "recall_labels.json")))
    out, tot = {}, {"off": [0, 0], "ladder": [0, 0]}
    for name in sorted(labels["streams"]):
        rows = labels["streams"][name]
        qs = W.queries(name, labels["n"])
        line = {}
        for knob, value in (("off", False), ("ladder", "ladder")):
            CM.fresh(M, value)
            t0 = time.perf_counter()
            got = CM.stream(M, qs)
            dt = time.perf_counter() - t0
            sat = [r["i"] for r in rows if r["label"] == "sat"]
            found = [i for i in sat if got[i] is not None]
            line[knob] = dict(counters(M), **{
                "sat_labelled": len(sat), "found": len(found),
                "missed": sorted(set(sat) - set(found)),
                "unsat_with_model": [r["i"] for r in rows
                                     if r["label"] == "unsat" and got[r["i"]] is not None],
                "wrong_models": [i for i, a in enumerate(got) if a is not None and
                                 R.eval_constraints(list(qs[i]), R.Assignment(
                                     a.vars, a.arrays, a.funcs)) != 1],
                "models": sum(a is not None for a in got), "wall_s": round(dt, 3)})
            tot[knob][0] += len(found)
            tot[knob][1] += len(sat)
        out[name] = line
        print("recall", name, json.dumps(line), flush=True)
    out["total"] = tot
    print("recall total", tot, flush=True)
    return out


def compiles(M, W, CY):
    out = {}
    orig = CY.compile_eval_ck
    log = []

    def traced(nodes, asg, sizes=None):
        n0 = len(CY._EVAL_CACHE)
        t = time.perf_counter()
        p = orig(nodes, asg, sizes)
        if len(CY._EVAL_CACHE) != n0:                    # compiled, not cached
            log.append({"ms": round((time.perf_counter() - t) * 1e3, 2),
                        "constraints": len(nodes), "witness_tables": CY.table_sizes(asg),
                        "table_sizes": CY.table_sizes_ck(nodes, asg),
                        "records": int(p.n_ins), "leaves": len(p.leaves)})
        return p
    CY.compile_eval_ck = traced
    try:
        for name, n in (("c4", 128), ("c5", 256)):
            qs = W.queries(name, n)
            CM.fresh(M, "ladder")
            del log[:]
            t0 = time.perf_counter()
            got = CM.stream(M, qs)
            out[name] = dict(counters(M), models=sum(a is not None for a in got),
                             wall_s=round(time.perf_counter() - t0, 3), compiles=len(log),
                             total_ms=round(sum(r["ms"] for r in log), 2),
                             dearest=max(log, key=lambda r: r["ms"]) if log else None)
            print("compile", name, json.dumps(out[name]), flush=True)
    finally:
        CY.compile_eval_ck = orig
    return out


def kernel_times(eng):
    """One call on a 33-root ladder over three 16-bit symbols; the rungs pin
    nothing, x, and x and y."""
    from mythril_amd.engine import default_leafgen
    from mythril_amd.ir import compile_constraints
    from mythril_amd.smt import node as N
    x, y, z = (N.bv_var(s, 16) for s in ("kx", "ky", "kz"))
    cs = [N.bv_cmp("bvult", x, N.bv_num(65535 - k * 1985, 16)) for k in range(31)]
    cs += [N.bv_cmp("bvult", y, N.bv_num(1 << 15, 16)), N.distinct(y, z)]
    prog = compile_constraints(cs)
    lp = eng.load(prog, default_leafgen(prog), prog_seed=3)
    n = len(prog.leaves)
    rows = np.zeros((n, 8), np.uint32)
    masks = np.array([[3], [1], [0]], np.uint32)

    def timed(call):
        ms, wall = [], []
        for _ in range(12):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(eng.last_kernel_ms())
        return {"kernel_ms_median": float(np.median(ms[2:])),
                "wall_ms_median": float(np.median(wall[2:]))}
    out = {}
    for jobs in (1, 64, 256):
        for n_rungs in (1, 3):
            m = masks[3 - n_rungs:]
            key = "%d jobs x 256 lanes x %d rungs" % (jobs, n_rungs)
            out[key] = {
                "carry_ladder": timed(lambda: eng.carry_ladder([(lp, rows, m)] * jobs, 1, 0, 256)),
                "carry_batch_same_columns": timed(
                    lambda: eng.carry_batch([(lp, rows, m[-1])] * jobs, 1, 0, 256 * n_rungs))}
            print("kernel", key, json.dumps(out[key]), flush=True)
    return out


def main():
    import mythril_amd.model as M
    from mythril_amd import carry as CY
    from mythril_amd import workloads as W
    from mythril_amd.engine import get_engine
    from oracle import smtlib_ref as R                   # checker only
    M.time_handler.start_execution(36000)
    res = {"kernel": kernel_times(get_engine(0))}
    res["recall"] = recall(M, W, R)
    res["compile"] = compiles(M, W, CY)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Witness sets on the pin ladder, in one process
on the GPU; the helpers are those of tools/carry_measure.py.

* --kernel -- device time (``Engine.last_kernel_ms``, median of 10) of one
  ``Engine.carry_ladder_sets`` call beside ``Engine.carry_ladder`` in the same
  run at 1, 64 and 256 jobs x 256 lanes x 1, 3 and 8 rungs (round 17's 33-root
  ladder program); the sets call reads 1 row set at 1 rung, 2 at 3 and 4 at 8.
* --recall -- every labelled stream of tests/golden/recall_labels.json in order
  through ``get_model`` with the knob off and with ``MYTHRIL_GPU_CARRY=4``.

Usage:  python tools/carry_sets_measure.py [--kernel] [--recall] [out.json]
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


def kernel_times(eng):
    from mythril_amd.engine import default_leafgen
    from mythril_amd.ir import compile_constraints
    from mythril_amd.smt import node as N
    x, y, z = (N.bv_var(s, 16) for s in ("kx", "ky", "kz"))
    cs = [N.bv_cmp("bvult", x, N.bv_num(65535 - k * 1985, 16)) for k in range(31)]
    cs += [N.bv_cmp("bvult", y, N.bv_num(1 << 15, 16)), N.distinct(y, z)]
    prog = compile_constraints(cs)
    lp = eng.load(prog, default_leafgen(prog), prog_seed=3)
    n = len(prog.leaves)
    # every rung pins x to a row no candidate satisfies the ladder with, so no
    # job ends early on a hit and every column is evaluated
    ladder = np.array([[3], [1], [1], [3], [1], [3], [1], [1]], np.uint32)

    def timed(call):
        ms = []
        for _ in range(12):
            call()
            ms.append(eng.last_kernel_ms())
        return float(np.median(ms[2:]))
    out = {}
    for jobs in (1, 64, 256):
        for n_rungs, n_sets in ((1, 1), (3, 2), (8, 4)):
            m = ladder[:n_rungs]
            rows = np.zeros((n_sets, n, 8), np.uint32)
            rows[:, :, 0] = 0xFFFF                      # x = 65535 fails every threshold
            rung_set = (np.arange(n_rungs) % n_sets).astype(np.uint32)
            key = "%d jobs x 256 lanes x %d rungs" % (jobs, n_rungs)
            out[key] = {
                "sets": n_sets,
                "carry_ladder_ms": timed(lambda: eng.carry_ladder([(lp, rows[0], m)] * jobs, 1, 0,
                                                                  256)),
                "carry_ladder_sets_ms": timed(lambda: eng.carry_ladder_sets(
                    [(lp, rows, m, rung_set)] * jobs, 1, 0, 256))}
            print("kernel", key, json.dumps(out[key]), flush=True)
    return out


def recall(M, W, R):
    labels = json.load(open(os.path.join(ROOT, "tests", "golden", "recall_labels.json")))
    out, tot = {}, {"off": [0, 0], "sets": [0, 0]}
    for name in sorted(labels["streams"]):
        rows = labels["streams"][name]
        qs = W.queries(name, labels["n"])
        line = {}
        for knob, value in (("off", False), ("sets", "sets")):
            CM.fresh(M, value)
            t0 = time.perf_counter()
            got = CM.stream(M, qs)
            dt = time.perf_counter() - t0
            sat = [r["i"] for r in rows if r["label"] == "sat"]
            found = [i for i in sat if got[i] is not None]
            line[knob] = dict(CM.counters(M), **{
                "rung_hits": list(M.stats.carry_rung_hits),
                "set_hits": list(M.stats.carry_set_hits),
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


def main():
    import mythril_amd.model as M
    from mythril_amd import workloads as W
    from mythril_amd.engine import get_engine
    from oracle import smtlib_ref as R                   # checker only
    args = [a for a in sys.argv[1:] if a.startswith("--")]
    paths = [a for a in sys.argv[1:] if not a.startswith("--")]
    M.time_handler.start_execution(36000)
    res = {}
    if "--kernel" in args:
        res["kernel"] = kernel_times(get_engine(0))
    if "--recall" in args:
        res["recall"] = recall(M, W, R)
    if paths:
        with open(paths[0], "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

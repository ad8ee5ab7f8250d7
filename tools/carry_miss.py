#!/usr/bin/env python3
"""Why the pin ladder misses, in one process on
the GPU; the helpers are those of tools/carry_measure.py.

* miss (default) -- the c1, c4 and c5 streams through ``get_model`` under the
  ladder with ``carry.run_census`` in place of ``carry.run_ladder``: for every
  extension that misses on every rung the rung names, per rung the worst
  blocker (``Census.blockers()[0]``) with its constraint text and its ``pass``
  / ``sole_block`` counts, and start 0's failing roots; then per stream the
  misses counted by the kind of the worst blocker, per rung: a constraint the
  extension adds ("new") or one of the remembered groups ("parent").
* --kernel -- device time (``Engine.last_kernel_ms``, median of 10) of one
  ``Engine.carry_census`` call beside ``Engine.carry_ladder`` in the same run at
  1, 64 and 256 jobs x 256 lanes x 1 and 3 rungs, 4 walkers.
* --recall -- every labelled stream of tests/golden/recall_labels.json in order
  through ``get_model`` with the knob off and with ``MYTHRIL_GPU_CARRY=3``.

Usage:  python tools/carry_miss.py [--kernel] [--recall] [--no-miss] [out.json]
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

STREAMS = (("c1", 128), ("c4", 128), ("c5", 256))


def misses(M, W, CY):
    out = {}
    log = []
    orig = CY.run_ladder

    def censused(eng, items, seed, leafgen, lanes=None, phase=None):
        res = CY.run_census(eng, items, seed, leafgen, lanes, M.CARRY_WALKERS, phase)
        back = []
        for (nodes, _, taken), r in zip(items, res):
            if r is None:
                back.append(None)
                continue
            n = sum(int(c.n_cand) for c in r["censuses"])
            back.append((r["assignment"], r["program"], n, r["rung"]))
            if r["assignment"] is None:
                new = {x.id for x in CY.split_nodes(nodes, taken)[1]}
                rep = CY.miss_report(nodes, r["censuses"], r["kept"])
                log.append({"constraints": len(nodes), "new": len(new),
                            "start0_nfail": int(r["start_nfail"][0]),
                            "start0_rung": CY.RUNG_NAMES[r["kept"][int(r["start_col"][0]) //
                                                                   r["lanes"]]],
                            "rungs": [{"rung": q["rung"], "best_nfail": q["best_nfail"],
                                       "worst": dict(q["blockers"][0], kind=(
                                           "new" if nodes[q["blockers"][0]["root"]].id in new
                                           else "parent"))} for q in rep]})
        return back
    CY.run_ladder = censused
    try:
        for name, n in STREAMS:
            qs = W.queries(name, n)
            CM.fresh(M, "ladder")
            del log[:]
            got = CM.stream(M, qs)
            kinds = {}
            for m in log:
                for q in m["rungs"]:
                    k = kinds.setdefault(q["rung"], {"new": 0, "parent": 0})
                    k[q["worst"]["kind"]] += 1
            out[name] = dict(CM.counters(M), models=sum(a is not None for a in got),
                             misses=len(log), worst_blocker_kind=kinds,
                             start0_nfail=sorted(m["start0_nfail"] for m in log),
                             each=list(log))
            for m in log:
                print("miss", name, json.dumps(m)[:600], flush=True)
            print("summary", name, json.dumps({k: v for k, v in out[name].items() if k != "each"}),
                  flush=True)
    finally:
        CY.run_ladder = orig
    return out


def kernel_times(eng):
    """Round 17's shapes: a 33-root ladder over three 16-bit symbols, the rungs
    pin nothing, x, and x and y; here with its verdict mask as probe 0."""
    from mythril_amd import census as CS
    from mythril_amd.engine import default_leafgen
    from mythril_amd.ir import compile_constraints
    from mythril_amd.smt import node as N
    x, y, z = (N.bv_var(s, 16) for s in ("kx", "ky", "kz"))
    cs = [N.bv_cmp("bvult", x, N.bv_num(65535 - k * 1985, 16)) for k in range(31)]
    cs += [N.bv_cmp("bvult", y, N.bv_num(1 << 15, 16)), N.distinct(y, z)]
    prog = compile_constraints(cs, CS.mask_probes(cs))
    lp = eng.load(prog, default_leafgen(prog), prog_seed=3)
    rows = np.zeros((len(prog.leaves), 8), np.uint32)
    masks = np.array([[3], [1], [0]], np.uint32)

    def timed(call):
        ms = []
        for _ in range(12):
            call()
            ms.append(eng.last_kernel_ms())
        return float(np.median(ms[2:]))
    out = {}
    for jobs in (1, 64, 256):
        for n_rungs in (1, 3):
            m = masks[3 - n_rungs:]
            key = "%d jobs x 256 lanes x %d rungs" % (jobs, n_rungs)
            out[key] = {
                "carry_ladder_ms": timed(lambda: eng.carry_ladder([(lp, rows, m)] * jobs, 1, 0,
                                                                  256)),
                "carry_census_ms": timed(lambda: eng.carry_census(
                    [(lp, rows, m, len(cs))] * jobs, 1, 0, 256, 4))}
            print("kernel", key, json.dumps(out[key]), flush=True)
    return out


def recall(M, W, R):
    labels = json.load(open(os.path.join(ROOT, "tests", "golden", "recall_labels.json")))
    out, tot = {}, {"off": [0, 0], "walk": [0, 0]}
    for name in sorted(labels["streams"]):
        rows = labels["streams"][name]
        qs = W.queries(name, labels["n"])
        line = {}
        for knob, value in (("off", False), ("walk", "walk")):
            CM.fresh(M, value)
            t0 = time.perf_counter()
            got = CM.stream(M, qs)
            dt = time.perf_counter() - t0
            sat = [r["i"] for r in rows if r["label"] == "sat"]
            found = [i for i in sat if got[i] is not None]
            line[knob] = dict(CM.counters(M), **{
                "rung_hits": list(M.stats.carry_rung_hits),
                "walk_attempts": M.stats.carry_walk_attempts,
                "walk_hits": M.stats.carry_walk_hits,
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
    from mythril_amd import carry as CY
    from mythril_amd import workloads as W
    from mythril_amd.engine import get_engine
    from oracle import smtlib_ref as R                   # checker only
    args = [a for a in sys.argv[1:] if a.startswith("--")]
    paths = [a for a in sys.argv[1:] if not a.startswith("--")]
    M.time_handler.start_execution(36000)
    res = {}
    if "--kernel" in args:
        res["kernel"] = kernel_times(get_engine(0))
    if "--no-miss" not in args:
        res["miss"] = misses(M, W, CY)
    if "--recall" in args:
        res["recall"] = recall(M, W, R)
    if paths:
        with open(paths[0], "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The delta carry against the ladder and the
knob off, on the GPU; the helpers are those of tools/carry_measure.py.

* streams (default) -- round 17's stream protocol: six fresh processes with
  ``MYTHRIL_GPU_CARRY`` at 0 / 2 / 5 / 0 / 2 / 5, each running the c1, c3, c4 and
  c5 stand-in streams through ``get_model`` one query at a time (the distinct
  queries among the first 128 of a stream; 16 of them cold first, every memo
  cleared before each, as tools/search_bench.py does, then the whole sample on
  kept memos).  Per stream and process: median, mean and max ms per query, the
  compile phase's ms per query, kernel launches and kernel ms per query, exact /
  attempts / hits, hits per rung of the ladder and of the delta, the groups the
  delta refused, and the roots the delta compiled against the roots of those
  groups.  Then a table of the six, and per stream whether knob 5's mean lies
  below knob 0's by more than the spread between the two runs of one knob.
* --recall -- every labelled stream of tests/golden/recall_labels.json in order
  through ``get_model`` with the knob off and with ``MYTHRIL_GPU_CARRY=5``, in
  this process.

Usage:  python tools/carry_delta_measure.py [--recall] [--no-streams] [out.json]
"""

import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import carry_measure as CM  # noqa: E402

KNOBS = ("0", "2", "5", "0", "2", "5")
STREAMS = ("c1", "c3", "c4", "c5")
QUERIES = 128


def delta_counters(M):
    s = M.stats
    return dict(CM.counters(M), rung_hits=list(s.carry_rung_hits),
                delta_attempts=s.carry_delta_attempts, delta_hits=list(s.carry_delta_hits),
                delta_ineligible=s.carry_delta_ineligible, delta_roots=s.carry_delta_roots,
                delta_group_roots=s.carry_delta_group_roots)


def child():
    """One process of the protocol, the knob from the environment: a JSON line
    per stream."""
    import mythril_amd.model as M
    from mythril_amd import workloads as W
    M.time_handler.start_execution(36000)
    for name in STREAMS:
        sample, seen = [], set()
        for q in W.queries(name, QUERIES):
            key = tuple(c.id for c in q)
            if key not in seen:
                seen.add(key)
                sample.append(q)

        def run(clear_each):
            lat, misses = [], 0
            M.stats.reset_gpu()
            M.clear_search_memos()
            for q in (sample[:16] if clear_each else sample):
                M.get_model.cache_clear()
                if clear_each:
                    M.clear_search_memos()
                t0 = time.perf_counter()
                try:
                    M.get_model(tuple(q), enforce_execution_time=False)
                except (M.SolverUnavailable, M.UnsatError):
                    misses += 1
                lat.append((time.perf_counter() - t0) * 1000.0)
            n = len(lat)
            return dict(delta_counters(M), stream=name, knob=os.environ.get("MYTHRIL_GPU_CARRY"),
                        queries=n, median_ms=statistics.median(lat), mean_ms=statistics.mean(lat),
                        max_ms=max(lat), gpu_misses=misses,
                        compile_ms_per_query=M.stats.phase["compile"] * 1000.0 / n,
                        kernel_ms_per_query=M.stats.kernel_time * 1000.0 / n,
                        launches_per_query=M.stats.launches / n)
        run(True)
        print("stream " + json.dumps(run(False)), flush=True)


def streams():
    runs = []
    for knob in KNOBS:
        env = dict(os.environ, MYTHRIL_GPU_CARRY=knob)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env,
                           stdout=subprocess.PIPE, universal_newlines=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit("knob %s: exit status %d" % (knob, p.returncode))
        got = [json.loads(l[7:]) for l in p.stdout.splitlines() if l.startswith("stream ")]
        for r in got:
            print("stream", json.dumps(r), flush=True)
        runs.append(got)
    by = {}
    for got in runs:
        for r in got:
            by.setdefault((r["stream"], r["knob"]), []).append(r)

    def pair(rs, k, fmt="%.3f"):
        return " / ".join(fmt % r[k] for r in rs)
    print("| stream | queries | knob | median | mean | max | compile | launches | exact / attempts "
          "/ hits | ladder rungs | delta attempts / hits | ineligible | roots | GPU misses |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    verdicts = {}
    for name in STREAMS:
        for knob in ("0", "2", "5"):
            rs = by[(name, knob)]
            r = rs[0]
            print("| %s | %d | %s | %s | %s | %s | %s | %.2f | %d / %d / %d | %s | %d / %s | %d | "
                  "%d of %d | %d |" % (
                      name if knob == "0" else "", r["queries"], knob, pair(rs, "median_ms"),
                      pair(rs, "mean_ms"), pair(rs, "max_ms", "%.2f"),
                      pair(rs, "compile_ms_per_query"), r["launches_per_query"], r["exact"],
                      r["attempts"], r["hits"], "/".join(map(str, r["rung_hits"])),
                      r["delta_attempts"], "/".join(map(str, r["delta_hits"])),
                      r["delta_ineligible"], r["delta_roots"], r["delta_group_roots"],
                      r["gpu_misses"]))
        means = {k: [r["mean_ms"] for r in by[(name, k)]] for k in ("0", "2", "5")}
        spread = max(max(v) - min(v) for v in means.values())
        gap = statistics.mean(means["0"]) - statistics.mean(means["5"])
        verdicts[name] = {"spread_ms": spread, "knob0_minus_knob5_mean_ms": gap,
                          "knob2_minus_knob5_mean_ms":
                              statistics.mean(means["2"]) - statistics.mean(means["5"]),
                          "knob5_below_knob0_by_more_than_the_spread": gap > spread}
        print("verdict", name, json.dumps(verdicts[name]), flush=True)
    return {"runs": runs, "verdicts": verdicts}


def recall(M, W, R):
    labels = json.load(open(os.path.join(ROOT, "tests", "golden", "recall_labels.json")))
    out, tot = {}, {"off": [0, 0], "delta": [0, 0]}
    for name in sorted(labels["streams"]):
        rows = labels["streams"][name]
        qs = W.queries(name, labels["n"])
        line = {}
        for knob, value in (("off", False), ("delta", "delta")):
            CM.fresh(M, value)
            t0 = time.perf_counter()
            got = CM.stream(M, qs)
            dt = time.perf_counter() - t0
            sat = [r["i"] for r in rows if r["label"] == "sat"]
            found = [i for i in sat if got[i] is not None]
            line[knob] = dict(delta_counters(M), **{
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
    args = [a for a in sys.argv[1:] if a.startswith("--")]
    paths = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--child" in args:
        return child()
    res = {}
    if "--no-streams" not in args:
        res["streams"] = streams()          # before this process opens the device
    if "--recall" in args:
        import mythril_amd.model as M
        from mythril_amd import workloads as W
        from oracle import smtlib_ref as R               # checker only
        M.time_handler.start_execution(36000)
        res["recall"] = recall(M, W, R)
    if paths:
        with open(paths[0], "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

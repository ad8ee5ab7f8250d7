#!/usr/bin/env python3
"""Why the witness search misses a query.

Per-constraint verdict census (mythril_amd/census.py): for
every independent group of the query, over --candidates candidates of its
search program, the ranked blockers (constraints no candidate satisfies, then
the constraints that alone keep candidates from being models), each with a
depth-3 s-expression, the pass rates, the histogram of failing constraints
per candidate, the best candidate's failing set, and the census time next to
the time of a plain Engine.search miss over the same count on the plain
search program.

usage: tools/miss_census.py --workload {c1,c3,c3o,c4,c5} --query N
                            [--candidates K] [--json] [--split-and]
       tools/miss_census.py --known-misses [--candidates K] [--json] [--split-and]
           every entry of tests/golden/recall_known_miss.json and c3o query 50
       ... --repair [--lanes L] [--rounds R]
           after the census, the local search (mythril_amd/repair.py, DESIGN.md
           §3.9) from each launched group's best candidate: the trace, the
           outcome, and the device time per round next to the census's time
           for as many candidates in chunks of L
       ... --walk [--walkers N] [--lanes L] [--rounds R]
           after the census, the scored walk of N walkers
           (16) from each launched group's census starts: every walker's
           trace of (failing constraints, cost), the outcome, what the winner
           still fails, and the device time per round of one walker and of N
           beside mg_repair's on the same group
       ... --walk-tree [--walkers N] [--lanes L] [--rounds R]
           after the census, the same walk scored by distance trees (DESIGN.md
           §3.11): which scoring ran, roots by kind, simple or tree, atoms and
           residual probes, every walker's trace, the tree of each root the
           winner still fails (AND / OR / atoms with depth-3 s-expressions),
           and the device time per round beside mg_walk's and mg_repair's
       ... --walk-aim [--walkers N] [--lanes L] [--rounds R]
           after the census, the tree-scored walk with aimed moves (DESIGN.md
           §3.12): the aim table (per entry its residual probe, side, pieces
           and destination), per rule that refused a side of a HAMMING
           residual the number of sides and an example (--json: every side),
           every walker's trace, the tree of each root
           the winner still fails, and the device time per round beside
           mg_walk_tree's from the same starts
       ... --walk-bound [--walkers N] [--lanes L] [--rounds R]
           after the census, that walk with aims for orders too (DESIGN.md
           §3.13): the table's order entries (residual probe, mode, truth bit,
           pieces, fixed bits, destination), per order atom and simple order
           root the rule that refused each side without an entry, every
           walker's trace, the tree of each root the winner still fails, and
           the device time per round beside mg_walk_aim's from the same starts
       ... --walk-uf [--walkers N] [--lanes L] [--rounds R]
           after the census, that walk with aims for UF outputs too (DESIGN.md
           §3.14): the slots, how many sides of the read residuals resolve with
           and without them, per reason the refused sides, every walker's
           trace, and the device time per round beside scored="bound"
       ... --walk-sum [--walkers N] [--lanes L] [--rounds R]
           after the census, that walk with aims through sums, differences,
           masks and shifts too: the entries, the linear
           ones and their side rows, how many of the sides §3.14 refused now
           resolve or are linear and what refused them before, per reason the
           sides still refused, every walker's trace, and the device time per
           round beside scored="uf"
       tools/miss_census.py [workload] [n]
           the older census: which of a stream's first n queries the batched
           search misses, grouped by the shape of their newest constraint
"""
import argparse
import collections
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def by_shape(wl, n):
    import mythril_amd.model as M
    from mythril_amd import workloads as W
    from mythril_amd.engine import get_engine
    eng = get_engine(0)
    qs = W.queries(wl, n)
    progs, qmap = [], []
    for qi, q in enumerate(qs):
        for b in M.dependence_buckets(q):
            progs.append(M._compile_search(b))
            qmap.append(qi)
    loaded = [eng.load(p, M.search_leafgen(p), prog_seed=0) for p in progs]
    hits = eng.batch_search(loaded, M.SEARCH_SEED, M.SEARCH_CANDIDATES)
    solved = [True] * len(qs)
    first = collections.defaultdict(list)
    for qi, (i, _), p in zip(qmap, hits, progs):
        solved[qi] = solved[qi] and i >= 0
        first[qi].append(i)
    census = collections.Counter()
    for qi, q in enumerate(qs):
        if not solved[qi]:
            census[M.query_shape(q[-1])] += 1
    idx = sorted(i for v in first.values() for i in v if i >= 0)
    print(json.dumps({"workload": wl, "queries": n, "hits": sum(solved),
                      "first_index_median": idx[len(idx) // 2] if idx else None,
                      "first_index_max": idx[-1] if idx else None,
                      "missed_by_shape": census.most_common()}, indent=1))


def stream_query(wl, i):
    """Query ``i`` of a stream as the recall labels index it."""
    from mythril_amd import workloads as W
    n = json.load(open(os.path.join(GOLDEN, "recall_labels.json")))["n"]
    return W.queries(wl, max(n, i + 1))[i]


def plain_search_miss(group, n_cand, device=0):
    """(first index or -1, device ms, wall ms) of Engine.search over
    ``n_cand`` candidates of the group's plain search program."""
    import mythril_amd.model as M
    from mythril_amd.engine import get_engine
    prog = group["plain_program"]
    eng = get_engine(device, nreg=prog.nreg)
    lp = eng.load(prog, M.search_leafgen(prog), prog_seed=0)
    t0 = time.perf_counter()
    idx, _ = eng.search(lp, M.SEARCH_SEED, n_cand)
    return idx, eng.last_kernel_ms(), (time.perf_counter() - t0) * 1e3


def report(wl, qi, n_cand, split_and=False):
    """The JSON-able miss report of one stream query; ``split_and``: of the
    query with every top-level ``and`` replaced by its conjuncts (which half
    of a blocking constraint fails), ``labels`` naming each row "i.j" =
    conjunct j of constraint i."""
    from mythril_amd import census as CS
    from mythril_amd.smt import node as N
    q = stream_query(wl, qi)
    labels = [str(i) for i in range(len(q))]
    if split_and:
        parts = [(list(c.args) if c.op == "and" else [c]) for c in q]
        labels = ["%d.%d" % (i, j) if len(ps) > 1 else str(i)
                  for i, ps in enumerate(parts) for j in range(len(ps))]
        q = [p for ps in parts for p in ps]
    t0 = time.perf_counter()
    rep = CS.explain(q, n_cand=n_cand, form="search")
    out = {"workload": wl, "query": qi, "constraints": len(q), "candidates": n_cand,
           "split_and": split_and, "labels": labels,
           "explain_wall_ms": round((time.perf_counter() - t0) * 1e3, 1), "groups": []}
    for g in rep["groups"]:
        row = {"status": g["status"], "constraints": g["constraints"]}
        if "why" in g:
            row["why"] = g["why"]
        if g["status"] == CS.CENSUS:
            c = g["census"]
            pos = g["constraints"]
            k_of = {p: k for k, p in enumerate(pos)}
            row["records"] = g["records"]
            row["plain_records"] = g["plain_records"]
            row["n_sat"] = c.n_sat
            row["blockers"] = [
                {"constraint": p, "label": labels[p], "pass": int(c.pass_[k_of[p]]),
                 "pass_rate": round(int(c.pass_[k_of[p]]) / max(1, c.n_cand), 6),
                 "first_block": int(c.first_block[k_of[p]]),
                 "sole_block": int(c.sole_block[k_of[p]]),
                 "sole_index": int(c.sole_index[k_of[p]]),
                 "sexpr": N.to_sexpr(q[p], 3)} for p in g["blockers"]]
            row["pass_rates"] = {str(p): round(int(c.pass_[k]) / max(1, c.n_cand), 6)
                                 for k, p in enumerate(pos)}
            row["nfail_hist"] = {str(f): int(v) for f, v in enumerate(c.nfail_hist) if v}
            if "best" in g:
                a = g["best"]["assignment"]
                row["best"] = {"index": g["best"]["index"], "nfail": g["best"]["nfail"],
                               "failing": g["best"]["failing"],
                               "vars": {k: hex(v) for k, v in sorted(a.vars.items())}}
            idx, ms, wall = plain_search_miss(g, n_cand)
            row["census_kernel_ms"] = round(c.kernel_ms, 3)
            row["plain_search"] = {"first_index": idx, "kernel_ms": round(ms, 3),
                                   "wall_ms": round(wall, 3)}
        out["groups"].append(row)
    return out


def repair_rows(wl, qi, n_cand, lanes, rounds):
    """Per independent group of the query: what ``repair.repair_group`` did
    (status, start, trace, rounds) and, for a group whose search ran, the
    device time per round beside ``Engine.census`` over rounds x lanes
    candidates of the same view in chunks of ``lanes``."""
    import mythril_amd.model as M
    from mythril_amd import census as CS
    from mythril_amd import repair as RP
    from mythril_amd.engine import get_engine
    rows = []
    for group in M.dependence_buckets(stream_query(wl, qi)):
        g = RP.repair_group(group, n_cand=n_cand, form="search", lanes=lanes, max_rounds=rounds)
        row = {"constraints": len(group), "status": g["status"]}
        if "why" in g:
            row["why"] = g["why"]
        if "start" in g:
            row["start"] = g["start"]
        res = g.get("repair")
        if res is not None:
            row.update(nfail=res.nfail, rounds=res.rounds,
                       trace=[int(v) for v in res.trace[:res.rounds]],
                       repair_kernel_ms=round(res.kernel_ms, 3),
                       ms_per_round=round(res.kernel_ms / max(1, res.rounds), 4))
            masked = CS._compile(group, CS.mask_probes(group), "search")
            eng = get_engine(0, nreg=masked.nreg)
            n_mask = CS.n_mask_probes(len(group))
            lp = eng.load(CS.census_view(masked, n_mask), CS._leafgen(masked, "search"), prog_seed=0)
            chunk = (lanes + 255) // 256 * 256
            c = eng.census(lp, M.SEARCH_SEED, 0, res.rounds * chunk, len(group), 0, chunk)
            row["census_same_candidates_ms"] = round(c.kernel_ms, 3)
            row["census_ms_per_chunk"] = round(c.kernel_ms / max(1, res.rounds), 4)
            row["records"] = masked.n_ins
        rows.append(row)
    return rows


def show_repair(rows, lanes):
    for gi, g in enumerate(rows):
        print(" repair group %d: %d constraints -> %s%s" % (
            gi, g["constraints"], g["status"], (" (%s)" % g["why"]) if "why" in g else ""))
        if "start" in g:
            print("  start: candidate %d, %d failing" % (g["start"]["index"], g["start"]["nfail"]))
        if "trace" in g:
            print("  %d rounds of %d lanes, %d failing at the end; trace: %s" % (
                g["rounds"], lanes, g["nfail"], " ".join(str(v) for v in g["trace"])))
            print("  device: %.3f ms, %.4f ms per round (%d records); census of the same %d "
                  "candidates in chunks of %d: %.3f ms, %.4f ms per chunk" % (
                      g["repair_kernel_ms"], g["ms_per_round"], g["records"],
                      g["rounds"] * lanes, lanes, g["census_same_candidates_ms"],
                      g["census_ms_per_chunk"]))


def _runs(trace):
    """A walker's trace [(nfail, cost), ...] as 'nfail/cost x rounds' runs."""
    out, prev, n = [], None, 0
    for key in [tuple(int(v) for v in t) for t in trace] + [None]:
        if key != prev and prev is not None:
            out.append("%d/%d" % prev + (" x%d" % n if n > 1 else ""))
            n = 0
        prev, n = key, n + 1
    return ", ".join(out)


def walk_rows(wl, qi, n_cand, lanes, rounds, walkers):
    """Per independent group of the query: what ``repair.repair_group(scored=
    True)`` did with ``walkers`` walkers (status, starts, every walker's
    trace, the roots the winner still fails with their kinds), and the device
    time per round of mg_walk with one walker and with ``walkers``, beside
    mg_repair's from the same start."""
    import mythril_amd.model as M
    from mythril_amd import repair as RP
    from mythril_amd.smt import node as N
    kinds = ("flat", "hamming", "magnitude")
    rows = []
    q = stream_query(wl, qi)
    where = {}
    for i, c in enumerate(q):
        where.setdefault(c.id, []).append(i)
    for group in M.dependence_buckets(q):
        pos = [where[c.id].pop(0) for c in group]        # root k = constraint pos[k]
        kw = dict(n_cand=n_cand, form="search", lanes=lanes, max_rounds=rounds)
        g = RP.repair_group(group, scored=True, walkers=walkers, **kw)
        row = {"constraints": len(group), "status": g["status"]}
        if "why" in g:
            row["why"] = g["why"]
        res = g.get("repair")
        if res is not None:
            t = g["table"]
            row.update(starts=g["starts"], winner=res.winner, rounds=res.rounds, walkers=walkers,
                       kinds={k: int((t >> 16 == i).sum()) for i, k in enumerate(kinds)},
                       residual_probes=len({int(v) & 0xFFFF for v in t if int(v) >> 16}),
                       nfail=[int(v) for v in res.nfail], cost=[int(v) for v in res.cost],
                       traces=[_runs(res.trace[w, :res.rounds]) for w in range(walkers)],
                       walk_kernel_ms=round(res.kernel_ms, 3),
                       walk_ms_per_round=round(res.kernel_ms / max(1, res.rounds), 4))
            row["failing"] = [{"root": k, "constraint": pos[k], "kind": kinds[int(t[k]) >> 16],
                               "sexpr": N.to_sexpr(group[k], 3)} for k in g.get("failing", [])]
            one = RP.repair_group(group, scored=True, walkers=1, **kw).get("repair")
            flat = RP.repair_group(group, **kw).get("repair")
            if one is not None:
                row["walk1_ms_per_round"] = round(one.kernel_ms / max(1, one.rounds), 4)
                row["walk1_rounds"] = one.rounds
            if flat is not None:
                row["repair_ms_per_round"] = round(flat.kernel_ms / max(1, flat.rounds), 4)
                row["repair_rounds"] = flat.rounds
        rows.append(row)
    return rows


def show_walk(rows, lanes):
    for gi, g in enumerate(rows):
        print(" walk group %d: %d constraints -> %s%s" % (
            gi, g["constraints"], g["status"], (" (%s)" % g["why"]) if "why" in g else ""))
        if "traces" not in g:
            continue
        print("  roots by kind: %s; %d residual probes" % (
            " ".join("%s %d" % kv for kv in g["kinds"].items()), g["residual_probes"]))
        print("  %d walkers, %d rounds of %d lanes each; winner: walker %d" % (
            g["walkers"], g["rounds"], lanes, g["winner"]))
        for w, tr in enumerate(g["traces"]):
            print("   walker %2d from candidate %d: ends %d/%d; nfail/cost per round: %s" % (
                w, g["starts"][w], g["nfail"][w], g["cost"][w], tr))
        for f in g["failing"]:
            print("  the winner still fails constraint #%d (root %d, %s): %s" % (
                f["constraint"], f["root"], f["kind"], f["sexpr"]))
        print("  device time per round: mg_walk x%d %.4f ms; mg_walk x1 %s ms; mg_repair %s ms" % (
            g["walkers"], g["walk_ms_per_round"], g.get("walk1_ms_per_round"),
            g.get("repair_ms_per_round")))


def tree_rows(wl, qi, n_cand, lanes, rounds, walkers):
    """Per independent group of the query: what ``repair.repair_group(scored=
    "tree")`` did with ``walkers`` walkers (which scoring ran, roots by kind,
    simple or tree, atoms and residual probes, every walker's trace, the tree
    of each root the winner still fails), and the device time per round of
    mg_walk_tree beside mg_walk's and mg_repair's from the same start."""
    import mythril_amd.model as M
    from mythril_amd import repair as RP
    from mythril_amd.smt import node as N
    kinds = ("flat", "hamming", "magnitude")
    rows = []
    q = stream_query(wl, qi)
    where = {}
    for i, c in enumerate(q):
        where.setdefault(c.id, []).append(i)
    for group in M.dependence_buckets(q):
        pos = [where[c.id].pop(0) for c in group]        # root k = constraint pos[k]
        kw = dict(n_cand=n_cand, form="search", lanes=lanes, max_rounds=rounds)
        g = RP.repair_group(group, scored="tree", walkers=walkers, **kw)
        row = {"constraints": len(group), "status": g["status"], "scoring": g.get("scoring")}
        if "why" in g:
            row["why"] = g["why"]
        res = g.get("repair")
        if res is not None:
            T = g.get("trees") or RP.simple_trees(g["table"])
            n_roots = len(group)
            simple = [k for k in range(n_roots) if not T.is_tree(k)]
            row.update(starts=g["starts"], winner=res.winner, rounds=res.rounds, walkers=walkers,
                       simple={k: sum(T.kind(r) == i for r in simple) for i, k in enumerate(kinds)},
                       trees=n_roots - len(simple), atoms=T.n_atoms,
                       atom_kinds={k: int((T.atoms >> 16 == i).sum()) for i, k in enumerate(kinds)},
                       residual_probes=len(T.probes) if g.get("trees") else None,
                       code_words=len(T.code),
                       nfail=[int(v) for v in res.nfail], cost=[int(v) for v in res.cost],
                       traces=[_runs(res.trace[w, :res.rounds]) for w in range(walkers)],
                       tree_kernel_ms=round(res.kernel_ms, 3),
                       tree_ms_per_round=round(res.kernel_ms / max(1, res.rounds), 4))
            row["failing"] = [{"root": k, "constraint": pos[k],
                               "tree": T.listing(k, 3, g.get("atom_state")) if T.is_tree(k) else
                               "simple %s: %s" % (kinds[T.kind(k)], N.to_sexpr(group[k], 3))}
                              for k in g.get("failing", [])]
            table = RP.repair_group(group, scored=True, walkers=walkers, **kw).get("repair")
            flat = RP.repair_group(group, **kw).get("repair")
            if table is not None:
                row["walk_ms_per_round"] = round(table.kernel_ms / max(1, table.rounds), 4)
                row["walk_rounds"] = table.rounds
            if flat is not None:
                row["repair_ms_per_round"] = round(flat.kernel_ms / max(1, flat.rounds), 4)
                row["repair_rounds"] = flat.rounds
        rows.append(row)
    return rows


def show_tree(rows, lanes):
    for gi, g in enumerate(rows):
        print(" tree walk group %d: %d constraints -> %s%s; scoring: %s" % (
            gi, g["constraints"], g["status"], (" (%s)" % g["why"]) if "why" in g else "",
            g["scoring"]))
        if "traces" not in g:
            continue
        print("  simple roots by kind: %s; %d tree roots, %d code words; atoms: %d (%s); "
              "%s residual probes" % (
                  " ".join("%s %d" % kv for kv in g["simple"].items()), g["trees"],
                  g["code_words"], g["atoms"],
                  " ".join("%s %d" % kv for kv in g["atom_kinds"].items()), g["residual_probes"]))
        print("  %d walkers, %d rounds of %d lanes each; winner: walker %d" % (
            g["walkers"], g["rounds"], lanes, g["winner"]))
        for w, tr in enumerate(g["traces"]):
            print("   walker %2d from candidate %d: ends %d/%d; nfail/cost per round: %s" % (
                w, g["starts"][w], g["nfail"][w], g["cost"][w], tr))
        for f in g["failing"]:
            print("  the winner still fails constraint #%d (root %d):" % (f["constraint"], f["root"]))
            for line in f["tree"].split("\n"):
                print("     " + line)
        print("  device time per round: mg_walk_tree x%d %.4f ms; mg_walk x%d %s ms; "
              "mg_repair %s ms" % (g["walkers"], g["tree_ms_per_round"], g["walkers"],
                                   g.get("walk_ms_per_round"), g.get("repair_ms_per_round")))


def aim_rows(wl, qi, n_cand, lanes, rounds, walkers):
    """Per independent group of the query: what ``repair.repair_group(scored=
    "aim")`` did with ``walkers`` walkers (the aim table, what refused the
    residuals without an entry, every walker's trace, the tree of each root the
    winner still fails), and the device time per round of mg_walk_aim beside
    mg_walk_tree's from the same starts."""
    import mythril_amd.model as M
    from mythril_amd import repair as RP
    from mythril_amd.smt import node as N
    kinds = ("flat", "hamming", "magnitude")
    rows = []
    q = stream_query(wl, qi)
    where = {}
    for i, c in enumerate(q):
        where.setdefault(c.id, []).append(i)
    for group in M.dependence_buckets(q):
        pos = [where[c.id].pop(0) for c in group]        # root k = constraint pos[k]
        kw = dict(n_cand=n_cand, form="search", lanes=lanes, max_rounds=rounds)
        g = RP.repair_group(group, scored="aim", walkers=walkers, **kw)
        row = {"constraints": len(group), "status": g["status"], "scoring": g.get("scoring")}
        if "why" in g:
            row["why"] = g["why"]
        res, T, A = g.get("repair"), g.get("trees"), g.get("aims")
        if res is not None and T is not None:
            row.update(starts=g["starts"], winner=res.winner, rounds=res.rounds, walkers=walkers,
                       atoms=T.n_atoms, residual_probes=len(T.probes),
                       nfail=[int(v) for v in res.nfail], cost=[int(v) for v in res.cost],
                       traces=[_runs(res.trace[w, :res.rounds]) for w in range(walkers)],
                       aim_kernel_ms=round(res.kernel_ms, 3),
                       aim_ms_per_round=round(res.kernel_ms / max(1, res.rounds), 4))
            row["entries"] = [{"probe": int(A.entries[e, 0]), "side": "ab"[A.sides[e]],
                               "pieces": int(A.entries[e, 2]),
                               "destination": N.to_sexpr(
                                   T.probes[int(A.entries[e, 0])].args[A.sides[e]], 3)}
                              for e in range(len(A))]
            prog = g["program"]
            used = sorted({int(e) & 0xFFFF for e in list(T.atoms) +
                           [r for r in T.roots if not int(r) & RP.WT_TREE]
                           if int(e) >> 16 == RP.HAMMING})
            have = {(int(A.entries[e, 0]), A.sides[e]) for e in range(len(A))}
            row["refused"] = []
            for p in used:
                for side, t in enumerate(T.probes[p].args):
                    if (p, side) in have:
                        continue
                    ps = RP.aim_pieces(t, prog)
                    why = RP.aim_refusal(t, prog) or (
                        "no piece" if not ps else "%d pieces" % len(ps) if len(ps) > 64 else
                        "a leaf the construction derives")
                    row["refused"].append({"probe": p, "side": "ab"[side], "why": why,
                                           "term": N.to_sexpr(t, 3)})
            row["failing"] = [{"root": k, "constraint": pos[k],
                               "tree": T.listing(k, 3, g.get("atom_state")) if T.is_tree(k) else
                               "simple %s: %s" % (kinds[T.kind(k)], N.to_sexpr(group[k], 3))}
                              for k in g.get("failing", [])]
            tree = RP.repair_group(group, scored="tree", walkers=walkers, **kw).get("repair")
            if tree is not None:
                row["tree_ms_per_round"] = round(tree.kernel_ms / max(1, tree.rounds), 4)
                row["tree_rounds"] = tree.rounds
                row["tree_end"] = [int(tree.nfail[tree.winner]), int(tree.cost[tree.winner])]
        rows.append(row)
    return rows


def show_aim(rows, lanes):
    for gi, g in enumerate(rows):
        print(" aimed walk group %d: %d constraints -> %s%s; scoring: %s" % (
            gi, g["constraints"], g["status"], (" (%s)" % g["why"]) if "why" in g else "",
            g["scoring"]))
        if "traces" not in g:
            continue
        print("  %d atoms, %d residual probes; aim table: %d entries" % (
            g["atoms"], g["residual_probes"], len(g["entries"])))
        for e in g["entries"]:
            print("   entry: residual %d side %s, %d pieces: %.160s" % (
                e["probe"], e["side"], e["pieces"], e["destination"]))
        # (--json lists every refused side; here one line per rule)
        rules = collections.OrderedDict()
        for e in g["refused"]:
            rules.setdefault(e["why"], []).append(e)
        for why, es in rules.items():
            print("   no entry: %d sides: %s, e.g. residual %d side %s: %.120s" % (
                len(es), why, es[0]["probe"], es[0]["side"], es[0]["term"]))
        print("  %d walkers, %d rounds of %d lanes each; winner: walker %d" % (
            g["walkers"], g["rounds"], lanes, g["winner"]))
        for w, tr in enumerate(g["traces"]):
            print("   walker %2d from candidate %d: ends %d/%d; nfail/cost per round: %s" % (
                w, g["starts"][w], g["nfail"][w], g["cost"][w], tr))
        for f in g["failing"]:
            print("  the winner still fails constraint #%d (root %d):" % (f["constraint"], f["root"]))
            for line in f["tree"].split("\n"):
                print("     " + line)
        print("  device time per round: mg_walk_aim x%d %.4f ms; mg_walk_tree x%d %s ms "
              "(%s rounds, ends %s)" % (g["walkers"], g["aim_ms_per_round"], g["walkers"],
                                        g.get("tree_ms_per_round"), g.get("tree_rounds"),
                                        g.get("tree_end")))


def bound_rows(wl, qi, n_cand, lanes, rounds, walkers):
    """Per independent group of the query: what ``repair.repair_group(scored=
    "bound")`` did with ``walkers`` walkers (the table's order entries, per
    order atom and simple order root what refused each side without an entry,
    every walker's trace, the tree of each root the winner still fails), and
    the device time per round of mg_walk_bound beside mg_walk_aim's from the
    same starts."""
    import mythril_amd.model as M
    from mythril_amd import repair as RP
    from mythril_amd.smt import node as N
    kinds = ("flat", "hamming", "magnitude")
    modes = ("xor", "low", "low_strict", "high", "high_strict")
    rows = []
    q = stream_query(wl, qi)
    where = {}
    for i, c in enumerate(q):
        where.setdefault(c.id, []).append(i)
    for group in M.dependence_buckets(q):
        pos = [where[c.id].pop(0) for c in group]        # root k = constraint pos[k]
        kw = dict(n_cand=n_cand, form="search", lanes=lanes, max_rounds=rounds)
        g = RP.repair_group(group, scored="bound", walkers=walkers, **kw)
        row = {"constraints": len(group), "status": g["status"], "scoring": g.get("scoring")}
        if "why" in g:
            row["why"] = g["why"]
        res, T, B = g.get("repair"), g.get("trees"), g.get("bounds")
        if res is not None and T is not None:
            row.update(starts=g["starts"], winner=res.winner, rounds=res.rounds, walkers=walkers,
                       atoms=T.n_atoms, residual_probes=len(T.probes),
                       nfail=[int(v) for v in res.nfail], cost=[int(v) for v in res.cost],
                       traces=[_runs(res.trace[w, :res.rounds]) for w in range(walkers)],
                       bound_kernel_ms=round(res.kernel_ms, 3),
                       bound_ms_per_round=round(res.kernel_ms / max(1, res.rounds), 4))
            row["xor_entries"] = len(B) - B.n_order
            row["entries"] = []
            for e in range(len(B)):
                p, _, cnt, mode, truth = (int(x) for x in B.entries[e])
                if mode == RP.BOUND_XOR:
                    continue
                row["entries"].append({
                    "probe": p, "mode": modes[mode], "pieces": cnt,
                    "truth": ("atom %d" % (truth & ~RP.BOUND_ATOM)) if truth & RP.BOUND_ATOM
                    else "root %d" % truth,
                    "fixed": "%#x" % B.fixed_of(e),
                    "destination": N.to_sexpr(T.probes[p].args[B.sides[e]], 3)})
            prog = g["program"]
            # every order atom, then every simple order root: the side without an entry
            orders = [("atom %d" % i, RP.order_sides(T.atom_nodes[i]))
                      for i, e in enumerate(T.atoms) if int(e) >> 16 == RP.MAGNITUDE]
            for k, c in enumerate(group):
                if not T.is_tree(k) and T.kind(k) == RP.MAGNITUDE:
                    d, neg = RP.peel(c)
                    orders.append(("root %d" % k, RP.order_sides(d, neg)))
            row["orders"] = len(orders)
            row["refused"] = []
            for name, sides in orders:
                if sides is None:
                    row["refused"].append({"order": name, "side": "-", "term": "",
                                           "why": "a simple root of the classify fallback"})
                    continue
                for side, t in zip(("lo", "hi"), sides[:2]):
                    if RP.bound_side(t, prog) is not None:
                        continue
                    ps = RP.aim_pieces(t, prog)
                    why = RP.aim_refusal(t, prog) or (
                        "no piece" if not ps else "%d pieces" % len(ps) if len(ps) > 64 else
                        "a leaf the construction derives")
                    row["refused"].append({"order": name, "side": side, "why": why,
                                           "term": N.to_sexpr(t, 3)})
            row["failing"] = [{"root": k, "constraint": pos[k],
                               "tree": T.listing(k, 3, g.get("atom_state")) if T.is_tree(k) else
                               "simple %s: %s" % (kinds[T.kind(k)], N.to_sexpr(group[k], 3))}
                              for k in g.get("failing", [])]
            aim = RP.repair_group(group, scored="aim", walkers=walkers, **kw).get("repair")
            if aim is not None:
                row["aim_ms_per_round"] = round(aim.kernel_ms / max(1, aim.rounds), 4)
                row["aim_rounds"] = aim.rounds
                row["aim_end"] = [int(aim.nfail[aim.winner]), int(aim.cost[aim.winner])]
        rows.append(row)
    return rows


def show_bound(rows, lanes):
    for gi, g in enumerate(rows):
        print(" bound walk group %d: %d constraints -> %s%s; scoring: %s" % (
            gi, g["constraints"], g["status"], (" (%s)" % g["why"]) if "why" in g else "",
            g["scoring"]))
        if "traces" not in g:
            continue
        print("  %d atoms, %d residual probes; table: %d XOR entries, %d order entries for %d "
              "orders" % (g["atoms"], g["residual_probes"], g["xor_entries"], len(g["entries"]),
                          g["orders"]))
        for e in g["entries"]:
            print("   entry: residual %d %s (%s), %d pieces, fixed %s: %.140s" % (
                e["probe"], e["mode"], e["truth"], e["pieces"], e["fixed"], e["destination"]))
        # (--json lists every refused side; here one line per rule)
        rules = collections.OrderedDict()
        for e in g["refused"]:
            rules.setdefault(e["why"], []).append(e)
        for why, es in rules.items():
            print("   no entry: %d sides: %s, e.g. %s side %s: %.120s" % (
                len(es), why, es[0]["order"], es[0]["side"], es[0]["term"]))
        print("  %d walkers, %d rounds of %d lanes each; winner: walker %d" % (
            g["walkers"], g["rounds"], lanes, g["winner"]))
        for w, tr in enumerate(g["traces"]):
            print("   walker %2d from candidate %d: ends %d/%d; nfail/cost per round: %s" % (
                w, g["starts"][w], g["nfail"][w], g["cost"][w], tr))
        for f in g["failing"]:
            print("  the winner still fails constraint #%d (root %d):" % (f["constraint"], f["root"]))
            for line in f["tree"].split("\n"):
                print("     " + line)
        print("  device time per round: mg_walk_%s x%d %.4f ms; mg_walk_aim x%d %s ms "
              "(%s rounds, ends %s)" % ("bound" if g["scoring"] == "bound" else "aim", g["walkers"],
                                        g["bound_ms_per_round"], g["walkers"],
                                        g.get("aim_ms_per_round"), g.get("aim_rounds"),
                                        g.get("aim_end")))


def uf_rows(wl, qi, n_cand, lanes, rounds, walkers):
    """Per independent group of the query: what ``repair.repair_group(scored=
    "uf")`` did with ``walkers`` walkers: the slots and their functions, how
    many sides of the read residual probes (both sides of every xor and
    difference a HAMMING or MAGNITUDE atom or simple root reads) resolve with
    the slots and how many did without, per reason the refused sides, every
    walker's trace, and the device time per round beside mg_walk_bound's (the
    same kernels on the table without slots) from the same starts."""
    import mythril_amd.model as M
    from mythril_amd import repair as RP
    from mythril_amd.smt import node as N
    rows = []
    for group in M.dependence_buckets(stream_query(wl, qi)):
        kw = dict(n_cand=n_cand, form="search", lanes=lanes, max_rounds=rounds)
        g = RP.repair_group(group, scored="uf", walkers=walkers, **kw)
        row = {"constraints": len(group), "status": g["status"], "scoring": g.get("scoring")}
        if "why" in g:
            row["why"] = g["why"]
        res, T, B, U = g.get("repair"), g.get("trees"), g.get("bounds"), g.get("ufs")
        if res is not None and T is not None:
            prog = g["program"]
            apps, _ = RP.uf_probes(T)
            row.update(starts=g["starts"], winner=res.winner, rounds=res.rounds, walkers=walkers,
                       nfail=[int(v) for v in res.nfail], cost=[int(v) for v in res.cost],
                       traces=[_runs(res.trace[w, :res.rounds]) for w in range(walkers)],
                       uf_ms_per_round=round(res.kernel_ms / max(1, res.rounds), 4),
                       applications=len(apps), slots=len(U), u_rows=int(U.n_urows),
                       functions=list(U.names), candidates=len(U.cands),
                       unwritable=int((U.cands[:, 0] == RP.AIM_NONE).sum()) if len(U.cands) else 0,
                       entries=len(B), slot_entries=sum(
                           any(leaf & RP.UF_SLOT for leaf, *_ in B.of(e)) for e in range(len(B))))
            slots = U.slot_of if len(U) else None
            sides = [t for p in RP._read_probes(T) if len(T.probes[p].args) == 2
                     for t in T.probes[p].args]
            row["sides"] = len(sides)
            row["resolved"] = sum(RP.aim_pieces(t, prog, slots) is not None for t in sides)
            row["resolved_without_slots"] = sum(RP.aim_pieces(t, prog) is not None for t in sides)
            row["refused"] = [{"why": RP.aim_refusal(t, prog, U if U.slot_of is not None else None),
                               "uf": t.op == "apply", "term": N.to_sexpr(t, 3)}
                              for t in sides if RP.aim_pieces(t, prog, slots) is None]
            bound = RP.repair_group(group, scored="bound", walkers=walkers, **kw).get("repair")
            if bound is not None:
                row["bound_ms_per_round"] = round(bound.kernel_ms / max(1, bound.rounds), 4)
                row["bound_rounds"] = bound.rounds
                row["bound_end"] = [int(bound.nfail[bound.winner]), int(bound.cost[bound.winner])]
        rows.append(row)
    return rows


def show_uf(rows, lanes):
    for gi, g in enumerate(rows):
        print(" uf walk group %d: %d constraints -> %s%s; scoring: %s" % (
            gi, g["constraints"], g["status"], (" (%s)" % g["why"]) if "why" in g else "",
            g["scoring"]))
        if "traces" not in g:
            continue
        print("  %d applications on the read sides, %d slots of %s, %d U rows; %d candidates, %d "
              "without a writable value leaf; %d entries, %d with a slot piece" % (
                  g["applications"], g["slots"], g["functions"], g["u_rows"], g["candidates"],
                  g["unwritable"], g["entries"], g["slot_entries"]))
        print("  sides of the read residuals: %d; resolve: %d (%d without slots); refused: %d, "
              "%d of them UF applications" % (g["sides"], g["resolved"],
                                              g["resolved_without_slots"], len(g["refused"]),
                                              sum(e["uf"] for e in g["refused"])))
        rules = collections.OrderedDict()
        for e in g["refused"]:
            rules.setdefault(e["why"], []).append(e)
        for why, es in rules.items():
            print("   refused: %d sides: %s, e.g. %.120s" % (len(es), why, es[0]["term"]))
        print("  %d walkers, %d rounds of %d lanes each; winner: walker %d" % (
            g["walkers"], g["rounds"], lanes, g["winner"]))
        for w, tr in enumerate(g["traces"]):
            print("   walker %2d from candidate %d: ends %d/%d; nfail/cost per round: %s" % (
                w, g["starts"][w], g["nfail"][w], g["cost"][w], tr))
        print("  device time per round: mg_walk_%s x%d %.4f ms; scored=\"bound\" x%d %s ms "
              "(%s rounds, ends %s)" % ("uf" if g["scoring"] == "uf" else g["scoring"],
                                        g["walkers"], g["uf_ms_per_round"], g["walkers"],
                                        g.get("bound_ms_per_round"), g.get("bound_rounds"),
                                        g.get("bound_end")))


def sum_rows(wl, qi, n_cand, lanes, rounds, walkers):
    """Per independent group of the query: what ``repair.repair_group(scored=
    "sum")`` did with ``walkers`` walkers: the entries, how many are linear and
    how many side rows they read, how many sides of the read residual probes
    resolve or are linear with an eligible target under the rules of DESIGN.md
    3.15 beside how many resolved under 3.14's, per reason the sides still
    refused, every walker's trace, and the device time per round beside
    scored="uf"'s (the same kernels on 3.14's table) from the same starts."""
    import mythril_amd.model as M
    from mythril_amd import repair as RP
    from mythril_amd.smt import node as N
    rows = []
    for group in M.dependence_buckets(stream_query(wl, qi)):
        kw = dict(n_cand=n_cand, form="search", lanes=lanes, max_rounds=rounds)
        g = RP.repair_group(group, scored="sum", walkers=walkers, **kw)
        row = {"constraints": len(group), "status": g["status"], "scoring": g.get("scoring")}
        if "why" in g:
            row["why"] = g["why"]
        res, T, B, U, S = (g.get(k) for k in ("repair", "trees", "bounds", "ufs", "sums"))
        if res is not None and T is not None:
            prog = g["program"]
            row.update(starts=g["starts"], winner=res.winner, rounds=res.rounds, walkers=walkers,
                       nfail=[int(v) for v in res.nfail], cost=[int(v) for v in res.cost],
                       traces=[_runs(res.trace[w, :res.rounds]) for w in range(walkers)],
                       sum_ms_per_round=round(res.kernel_ms / max(1, res.rounds), 4),
                       entries=len(B), linear=S.n_linear, side_rows=int(S.n_srows), slots=len(U))
            # (as sum_table resolves: an application at a numeral key only
            # where the table has slots)
            slots = U.slot_of if len(U) else None
            ufs = U if U.slot_of is not None else None
            sides = [t for p in RP._read_probes(T) if len(T.probes[p].args) == 2
                     for t in T.probes[p].args]
            row["sides"] = len(sides)

            def moves(t):
                terms = RP.linear_terms(t)
                return RP.aim_pieces(t, prog, slots, True) is not None or (
                    terms is not None and any(not isinstance(RP.sum_target(t, i, prog, slots), str)
                                              for i in range(len(terms))))
            old = [t for t in sides if RP.aim_pieces(t, prog, slots) is None]
            new = [t for t in sides if not moves(t)]
            row["refused_before"] = len(old)
            gained = [t for t in old if moves(t)]
            row["gained"] = [{"was": RP.aim_refusal(t, prog, ufs),
                              "linear": RP.linear_terms(t) is not None,
                              "term": N.to_sexpr(t, 3)} for t in gained]
            row["refused"] = [{"why": RP.aim_refusal(t, prog, ufs, True) or
                               "resolves only in a table that has slots", "uf": t.op == "apply",
                               "term": N.to_sexpr(t, 3)} for t in new]
            uf = RP.repair_group(group, scored="uf", walkers=walkers, **kw).get("repair")
            if uf is not None:
                row["uf_ms_per_round"] = round(uf.kernel_ms / max(1, uf.rounds), 4)
                row["uf_rounds"] = uf.rounds
                row["uf_end"] = [int(uf.nfail[uf.winner]), int(uf.cost[uf.winner])]
        rows.append(row)
    return rows


def show_sum(rows, lanes):
    for gi, g in enumerate(rows):
        print(" sum walk group %d: %d constraints -> %s%s; scoring: %s" % (
            gi, g["constraints"], g["status"], (" (%s)" % g["why"]) if "why" in g else "",
            g["scoring"]))
        if "traces" not in g:
            continue
        print("  %d entries, %d linear, %d side rows, %d slots" % (
            g["entries"], g["linear"], g["side_rows"], g["slots"]))
        print("  sides of the read residuals: %d; refused before: %d; of them now resolved or "
              "linear: %d; still refused: %d, %d of them UF applications" % (
                  g["sides"], g["refused_before"], len(g["gained"]), len(g["refused"]),
                  sum(e["uf"] for e in g["refused"])))
        was = collections.OrderedDict()
        for e in g["gained"]:
            was.setdefault((e["was"], e["linear"]), []).append(e)
        for (why, linear), es in was.items():
            print("   gained: %d sides (%s) that were: %s, e.g. %.120s" % (
                len(es), "linear" if linear else "pieces", why, es[0]["term"]))
        rules = collections.OrderedDict()
        for e in g["refused"]:
            rules.setdefault(e["why"], []).append(e)
        for why, es in rules.items():
            print("   refused: %d sides: %s, e.g. %.120s" % (len(es), why, es[0]["term"]))
        print("  %d walkers, %d rounds of %d lanes each; winner: walker %d" % (
            g["walkers"], g["rounds"], lanes, g["winner"]))
        for w, tr in enumerate(g["traces"]):
            print("   walker %2d from candidate %d: ends %d/%d; nfail/cost per round: %s" % (
                w, g["starts"][w], g["nfail"][w], g["cost"][w], tr))
        print("  device time per round: scored=\"sum\" (%s) x%d %.4f ms; scored=\"uf\" x%d %s ms "
              "(%s rounds, ends %s)" % (g["scoring"], g["walkers"], g["sum_ms_per_round"],
                                        g["walkers"], g.get("uf_ms_per_round"),
                                        g.get("uf_rounds"), g.get("uf_end")))


def show(r):
    print("== %s query %d%s: %d constraints, %d candidates per group (%.0f ms in all)" % (
        r["workload"], r["query"], " (top-level ands split, i.j = conjunct j of constraint i)"
        if r["split_and"] else "", r["constraints"], r["candidates"], r["explain_wall_ms"]))
    lab = r["labels"]
    for gi, g in enumerate(r["groups"]):
        print(" group %d: %d constraints %s -> %s%s" % (
            gi, len(g["constraints"]),
            " ".join([lab[p] for p in g["constraints"][:12]] + ["..."] * (len(g["constraints"]) > 12)),
            g["status"], (" (%s)" % g["why"]) if "why" in g else ""))
        if "blockers" not in g:
            continue
        print("  program: %d records with the mask (%d plain); satisfying candidates: %d" % (
            g["records"], g["plain_records"], g["n_sat"]))
        print("  census %.3f ms on the device; plain search miss %.3f ms (first index %d)" % (
            g["census_kernel_ms"], g["plain_search"]["kernel_ms"], g["plain_search"]["first_index"]))
        print("  blockers (worst first):")
        for b in g["blockers"]:
            print("   #%-5s pass %8d (%.4f)  first %8d  sole %8d  %s" % (
                b["label"], b["pass"], b["pass_rate"], b["first_block"], b["sole_block"],
                b["sexpr"]))
        always = [lab[int(p)] for p, v in g["pass_rates"].items() if v == 1.0]
        print("  always hold: %s" % " ".join(always))
        print("  failing constraints per candidate: %s" % "  ".join(
            "%s: %d" % fv for fv in g["nfail_hist"].items()))
        if "best" in g:
            print("  best candidate: index %d, %d failing: %s" % (
                g["best"]["index"], g["best"]["nfail"],
                " ".join(lab[p] for p in g["best"]["failing"])))


def main():
    if len(sys.argv) > 1 and not sys.argv[1].startswith("-"):
        return by_shape(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 64)
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--workload", choices=["c1", "c3", "c3o", "c4", "c5"])
    ap.add_argument("--query", type=int)
    ap.add_argument("--known-misses", action="store_true")
    ap.add_argument("--candidates", type=int, default=1 << 16)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--split-and", action="store_true",
                    help="census the query with every top-level `and` split into its conjuncts")
    ap.add_argument("--repair", action="store_true",
                    help="then run the local search from each group's best candidate")
    ap.add_argument("--walk", action="store_true",
                    help="then run the scored walk from each group's census starts")
    ap.add_argument("--walk-tree", action="store_true",
                    help="then run the walk scored by distance trees (DESIGN.md 3.11)")
    ap.add_argument("--walk-aim", action="store_true",
                    help="then run the tree-scored walk with aimed moves (DESIGN.md 3.12)")
    ap.add_argument("--walk-bound", action="store_true",
                    help="then run that walk with aims for orders too (DESIGN.md 3.13)")
    ap.add_argument("--walk-uf", action="store_true",
                    help="then run that walk with aims for UF outputs too (DESIGN.md 3.14)")
    ap.add_argument("--walk-sum", action="store_true",
                    help="then run that walk with aims through sums too (DESIGN.md 3.15)")
    ap.add_argument("--walkers", type=int, default=16)
    ap.add_argument("--lanes", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=64)
    a = ap.parse_args()
    if a.known_misses:
        known = json.load(open(os.path.join(GOLDEN, "recall_known_miss.json")))
        jobs = sorted({(wl, int(i)) for wl, rows in known.items() for i in rows} | {("c3o", 50)})
    elif a.workload is not None and a.query is not None:
        jobs = [(a.workload, a.query)]
    elif len(sys.argv) == 1:
        return by_shape("c4", 64)
    else:
        ap.error("give --workload and --query, or --known-misses")
    reports = [report(wl, qi, a.candidates, a.split_and) for wl, qi in jobs]
    if a.repair:
        for r in reports:
            r["repair"] = repair_rows(r["workload"], r["query"], a.candidates, a.lanes, a.rounds)
    if a.walk:
        for r in reports:
            r["walk"] = walk_rows(r["workload"], r["query"], a.candidates, a.lanes, a.rounds,
                                  a.walkers)
    if a.walk_tree:
        for r in reports:
            r["walk_tree"] = tree_rows(r["workload"], r["query"], a.candidates, a.lanes, a.rounds,
                                       a.walkers)
    if a.walk_aim:
        for r in reports:
            r["walk_aim"] = aim_rows(r["workload"], r["query"], a.candidates, a.lanes, a.rounds,
                                     a.walkers)
    if a.walk_bound:
        for r in reports:
            r["walk_bound"] = bound_rows(r["workload"], r["query"], a.candidates, a.lanes,
                                         a.rounds, a.walkers)
    if a.walk_uf:
        for r in reports:
            r["walk_uf"] = uf_rows(r["workload"], r["query"], a.candidates, a.lanes, a.rounds,
                                   a.walkers)
    if a.walk_sum:
        for r in reports:
            r["walk_sum"] = sum_rows(r["workload"], r["query"], a.candidates, a.lanes, a.rounds,
                                     a.walkers)
    if a.json:
        print(json.dumps(reports, indent=1))
    else:
        for r in reports:
            show(r)
            if a.repair:
                show_repair(r["repair"], a.lanes)
            if a.walk:
                show_walk(r["walk"], a.lanes)
            if a.walk_tree:
                show_tree(r["walk_tree"], a.lanes)
            if a.walk_aim:
                show_aim(r["walk_aim"], a.lanes)
            if a.walk_bound:
                show_bound(r["walk_bound"], a.lanes)
            if a.walk_uf:
                show_uf(r["walk_uf"], a.lanes)
            if a.walk_sum:
                show_sum(r["walk_sum"], a.lanes)


if __name__ == "__main__":
    main()

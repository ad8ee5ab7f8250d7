"""What the preparation of a repair_groups call costs with and without the job
axis, on one MI355X, all variants alternating in one run.

The groups: the first G (default 16) launched groups of the C4 stream in
search form, their census views and full masked programs loaded as
census.explain_group and repair._repair_steps load them.  Per walkers in
(1, 16), at n_cand = 2^16:
  seq_1, seq_2  G x (Engine.census + the Engine.witness calls of the group's
                distinct picks), as repair_group prepares
  batch         one Engine.census_batch + one Engine.batch_witness of all
                picks, as repair_groups prepares
  single, batch1  the first group alone, through the single calls and through
                a one-job batch
Prints device ms (kernel_ms of the census launches; the witness launches are
not in it on either side) and host wall ms per variant: median, min and max
over --calls calls (default 30).

``--ab-lib PATH``: Engine.census of the bench unit ("c4", 16) at 2^16
candidates through this tree's library and through another build of it (the
parent commit's), alternating, --calls calls each, twice per library: the
spread of each library's own repeats beside the difference between them."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np                                                   # noqa: E402
from mythril_amd import census as CS                                 # noqa: E402
from mythril_amd import engine as E                                  # noqa: E402
from mythril_amd import model as M                                   # noqa: E402
from mythril_amd.engine import default_leafgen, get_engine           # noqa: E402

N_CAND = 1 << 16


def report(label, runs):
    for key, v in runs.items():
        for what, col in (("device", 0), ("wall", 1)):
            x = [t[col] for t in v]
            print("%s x%d  %-8s %-6s ms: median %.4f min %.4f max %.4f"
                  % (label, len(x), key, what, statistics.median(x), min(x), max(x)))


def picks_of(c, walkers):
    """The starts repair._repair_steps picks from a census."""
    picks = [c.best_index]
    for k in c.blockers():
        if c.sole_index[k] >= 0 and int(c.sole_index[k]) not in picks:
            picks.append(int(c.sole_index[k]))
    return (picks + [c.best_index] * walkers)[:walkers]


def groups_of_c4(eng, want):
    """(view, full, n_roots) of the first `want` launched groups of the C4 stream."""
    from mythril_amd import workloads as W
    out = []
    for q in W.queries("c4", 64):
        for b in M.dependence_buckets(q):
            nodes = list(b)
            _, job = CS._explain_prepare(nodes, "search")
            if job is None or job[0].nreg != eng.nreg:
                continue
            masked, _, n_mask = job
            gens = CS._leafgen(masked, "search")
            out.append((eng.load(CS.census_view(masked, n_mask), gens, prog_seed=0),
                        eng.load(masked, gens, prog_seed=0), len(nodes)))
            if len(out) == want:
                return out
    return out


def prepare_time(G, calls):
    eng = get_engine(0, nreg=16)
    groups = groups_of_c4(eng, G)
    print("groups %d roots %s probes of the views %s" % (
        len(groups), [r for _, _, r in groups], [v.program.n_probes for v, _, _ in groups]))
    jobs = [(view, r, 0) for view, _, r in groups]
    for walkers in (1, 16):
        def seq(gs=groups):
            dev, out = 0.0, []
            for view, full, r in gs:
                c = eng.census(view, M.SEARCH_SEED, 0, N_CAND, r, 0)
                dev += c.kernel_ms
                rows = {}
                for i in picks_of(c, walkers):
                    if i not in rows:
                        rows[i] = eng.witness(full, M.SEARCH_SEED, i)[0]
                out.append((c, rows))
            return dev, out

        def batch(gs=groups, js=jobs):
            cs = eng.census_batch(js, M.SEARCH_SEED, 0, N_CAND)
            pairs = [(full, i) for (_, full, _), c in zip(gs, cs) for i in picks_of(c, walkers)]
            rows = eng.batch_witness(pairs, M.SEARCH_SEED, want_probes=False)
            return cs[0].kernel_ms, (cs, pairs, rows)
        single = lambda: seq(groups[:1])
        batch1 = lambda: batch(groups[:1], jobs[:1])
        # warm up, and the same censuses and rows
        (_, a), (_, (cs, pairs, rows)) = seq(), batch()
        at = 0
        for (c, single_rows), cb in zip(a, cs):
            assert c == cb
            for i in picks_of(cb, walkers):
                assert np.array_equal(rows[at][0], single_rows[i])
                at += 1
        print("walkers %d: witness launches %d single, 1 batched over %d pairs"
              % (walkers, sum(len(r) for _, r in a), len(pairs)))
        single(), batch1()
        plan = (("seq_1", seq), ("batch", batch), ("seq_2", seq), ("single", single),
                ("batch1", batch1))
        runs = {key: [] for key, _ in plan}
        for _ in range(calls):
            for key, fn in plan:
                t0 = time.perf_counter()
                dev, _ = fn()
                runs[key].append((dev, (time.perf_counter() - t0) * 1e3))
        report("groups %d walkers %2d n_cand 2^16" % (len(groups), walkers), runs)


def other_build(path, nreg=16):
    """An Engine on another build of the library that may lack this tree's newer
    entries: only what load and census call is declared."""
    lib = C.CDLL(path)
    p, u32, u64, i64 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int64
    lib.mg_init_layout.argtypes = [C.c_int, u32, C.POINTER(p)]
    lib.mg_free.argtypes, lib.mg_free.restype = [p], None
    lib.mg_last_error.argtypes, lib.mg_last_error.restype = [p], C.c_char_p
    lib.mg_load_program.argtypes = [p, p, u32, p, u32, p, u32, u32, u32, u64, C.POINTER(p)]
    lib.mg_free_program.argtypes, lib.mg_free_program.restype = [p], None
    lib.mg_census.argtypes = [p, p, C.POINTER(E.Gen), u64, u32, u32, u64, p, p, p, p, p,
                              C.POINTER(u32), C.POINTER(i64)]
    lib.mg_last_kernel_ms.argtypes, lib.mg_last_kernel_ms.restype = [p], C.c_float
    eng = E.Engine.__new__(E.Engine)
    eng.lib, eng.nreg = lib, nreg
    ctx = p()
    if lib.mg_init_layout(0, nreg, C.byref(ctx)) != 0:
        raise SystemExit("mg_init_layout failed on %s" % path)
    eng._ctx = ctx
    return eng


def single_ab(path, calls):
    import census_cases as K
    key = ("c4", 16)
    cs, prog = K.masked_program(key)
    engines = {"tree": get_engine(0, nreg=16), "other": other_build(path)}
    loaded = {k: e.load(prog, default_leafgen(prog), prog_seed=K.PROG_SEED)
              for k, e in engines.items()}
    run = lambda k: engines[k].census(loaded[k], K.SEED, 0, N_CAND, len(cs))
    assert run("tree") == run("other")                # warm up, and the same census
    plan = ("tree_1", "other_1", "tree_2", "other_2")
    runs = {key: [] for key in plan}
    for _ in range(calls):
        for key in plan:
            t0 = time.perf_counter()
            c = run(key.split("_")[0])
            runs[key].append((c.kernel_ms, (time.perf_counter() - t0) * 1e3))
    report("Engine.census c4/16 n_cand 2^16 (other = %s)" % os.path.basename(path), runs)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--groups", type=int, default=16)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--ab-lib", default=None)
    args = ap.parse_args()
    if args.ab_lib:
        single_ab(args.ab_lib, args.calls)
    else:
        prepare_time(args.groups, args.calls)

"""Device time per round of mg_walk_bound beside mg_walk_aim on the same
program, starts and XOR-only table (aim_cases `bytes`), in one run: aim, bound,
aim alternating.  Prints median, min and max of kernel_ms / rounds.
(mg_walk_uf and mg_walk_sum run mg_walk_bound's kernels: there is nothing to
time them against.)
``--batch G``: one Engine.walk_batch of G jobs beside G sequential
Engine.walk_sum calls (measured twice) and a one-job batch beside the single
walk, on the same program and table, 8 rounds per call, all variants
alternating in one run, 40 calls each: device time (kernel_ms, summed over the
sequential calls) and host wall time of the G walks, per round."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np                                                   # noqa: E402
import aim_cases as AC                                               # noqa: E402
from mythril_amd import repair as RP                                 # noqa: E402
from mythril_amd.engine import default_leafgen, get_engine           # noqa: E402

name = "bytes"
prog, T, A = AC.program(name), AC.trees(name), AC.aims(name)
n_roots = len(AC.case(name)[0])
B = RP.bounds_of_aims(A, n_roots, T.n_atoms)
eng = get_engine(0, nreg=16)
lp = eng.load(prog, default_leafgen(prog), prog_seed=0)
if "--batch" in sys.argv:
    import time
    G = int(sys.argv[sys.argv.index("--batch") + 1])
    none, sums = RP.no_ufs(), RP.no_sums(len(B))
    for walkers in (1, 16):
        starts = AC.starts(name, walkers)
        # other seeds per job: the jobs do not walk in step
        jobs = [(lp, starts, n_roots, T, B, none, sums, AC.SEED + g) for g in range(G)]
        one = lambda j: eng.walk_sum(j[0], j[1], j[2], T, B, none, sums, j[7], 4096, 8)

        def seq():
            return [one(j) for j in jobs]

        def timed(fn):
            """(device ms, wall ms, rounds) of the walks one call of fn makes"""
            t0 = time.perf_counter()
            res = fn()
            wall = (time.perf_counter() - t0) * 1e3
            res = res if isinstance(res, list) else [res]
            # a batch reports the device time of its launch sequence in every result
            dev = res[0].kernel_ms if fn in (batch, batch1) else sum(r.kernel_ms for r in res)
            return dev, wall, max(r.rounds for r in res)
        batch = lambda: eng.walk_batch(jobs, 4096, 8)
        batch1 = lambda: eng.walk_batch(jobs[:1], 4096, 8)
        single = lambda: one(jobs[0])
        for a, b in zip(batch(), seq()):                             # warm up, and the same walks
            assert np.array_equal(a.leaves, b.leaves) and np.array_equal(a.trace, b.trace)
            assert a.rounds == b.rounds
        plan = (("seq%d_1" % G, seq), ("batch%d" % G, batch), ("seq%d_2" % G, seq),
                ("single", single), ("batch1", batch1))
        runs = {key: [] for key, _ in plan}
        for _ in range(40):
            for key, fn in plan:
                dev, wall, rounds = timed(fn)
                runs[key].append((dev / rounds, wall / rounds))
        for key, v in runs.items():
            for what, col in (("device", 0), ("wall", 1)):
                x = [t[col] for t in v]
                print("walkers %2d lanes 4096 rounds 8 x40  %-9s %-6s ms/round: median %.4f "
                      "min %.4f max %.4f" % (walkers, key, what, statistics.median(x), min(x),
                                             max(x)))
    sys.exit(0)
for walkers in (1, 16):
    starts = AC.starts(name, walkers)
    aim = lambda: eng.walk_aim(lp, starts, n_roots, T, A, AC.SEED, 4096, 64)
    bound = lambda: eng.walk_bound(lp, starts, n_roots, T, B, AC.SEED, 4096, 64)
    plan = (("aim_1", aim), ("bound", bound), ("aim_2", aim))
    a, b = aim(), bound()                                            # warm up, and the same walk
    assert np.array_equal(a.leaves, b.leaves) and np.array_equal(a.trace, b.trace)
    assert a.rounds == b.rounds
    runs = {key: [] for key, _ in plan}
    for _ in range(40):
        for key, fn in plan:
            res = fn()
            runs[key].append(res.kernel_ms / res.rounds)
    for key, v in runs.items():
        print("walkers %2d lanes 4096 rounds %d x40  %-7s ms/round: median %.4f min %.4f max %.4f"
              % (walkers, a.rounds, key, statistics.median(v), min(v), max(v)))

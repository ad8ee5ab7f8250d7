#!/usr/bin/env python3
"""First GPU contact of a compiled-program build: a few corpus DAGs through
mg_batch_eval_gen on the interpreter and on their compiled code; root bits
and first indices must be identical.  Exits non-zero on any difference."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import bench  # noqa: E402
from mythril_amd import jit  # noqa: E402

n_dags = int(sys.argv[1]) if len(sys.argv) > 1 else 16
corpus = bench.build_corpus(n_dags, 8)
image = jit.compile_batch([(p, None, d) for d, p, _, _ in corpus], workers=8)
print("image %.1f MB" % (len(image) / 1e6), flush=True)

from gpu_batch import run_batch  # noqa: E402
from mythril_amd.engine import Engine  # noqa: E402
eng = Engine(0)
items = [(d, p) for d, p, _, _ in corpus]
N, FIRST = 1 << 12, (3 << 20) + 192

bi, fi = run_batch(eng, items, bench.SEED, FIRST, N)
print("interpreter done", flush=True)
bj, fj = run_batch(eng, items, bench.SEED, FIRST, N, image)
print("jit done", flush=True)
same = np.array_equal(bi, bj) and fi == fj
print("identical:", same, "sat lanes", int(bi.sum()))
for k in range(len(corpus)):
    if not np.array_equal(bi[k], bj[k]):
        diff = np.flatnonzero(bi[k] != bj[k])[:10]
        print("  dag", corpus[k][0], "lanes", diff.tolist(), "interp bits",
              bi[k][diff].astype(int).tolist())
sys.exit(0 if same else 1)

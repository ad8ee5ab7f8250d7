"""The simplifying lowering on the MI355X.

* the named rule cases of tests/test_simplify.py as one batch per register
  layout: 320 lanes of host leaves (a full workgroup and a partial one), the
  interpreter and the compiled code, every probe and root bit against
  ``oracle/evalref``;
* the 8 C2 bench units whose programs fold most, in generator mode through
  the parity tests' batch harness (tests/gpu_batch.py): 2^10 candidates from
  first index (3 << 20) + 192, root-bit rows and first satisfying indices
  with the pass on == with it off == ``oracle/evalref``.
"""

import numpy as np
import pytest

import bench
import gpu_batch as G
import test_simplify as T
from mythril_amd import jit
from mythril_amd.assign import Assignment as PA, pack
from mythril_amd.build import LAYOUT_LDS_SLOTS
from mythril_amd.ccompile import compile_native
from mythril_amd.engine import get_engine, limbs_to_int

pytestmark = pytest.mark.gpu
LANES = 320
N_LANES, FIRST = 1 << 10, (3 << 20) + 192


@pytest.mark.parametrize("nreg", [16, 11])
def test_rule_cases_host_leaves(nreg):
    engine = get_engine(0, nreg=nreg)
    names = sorted(T.CASES)
    asgs = T.assignments(LANES)
    assert len(asgs) == LANES
    progs = [T.compiled(name, nreg, True) for name in names]
    assert all(p.stats["folded"] > 0 for p in progs)
    inputs = [pack(p, [PA(vars=a) for a in asgs]) for p in progs]
    loaded = [engine.load(p) for p in progs]
    image = jit.compile_batch([(p, None, 0) for p in progs], workers=8, start="spawn",
                              lds_slots=LAYOUT_LDS_SLOTS[nreg])
    for path in ("interp", "jit"):
        handle = engine.jit_attach(loaded, image) if path == "jit" else None
        try:
            for name, p, lp, soa in zip(names, progs, loaded, inputs):
                roots, pr = engine.eval(lp, soa, want_probes=True)
                for a, (bit, vals) in enumerate(T.expected(name, asgs)):
                    got = [limbs_to_int(pr[k, :, a]) for k in range(p.n_probes)]
                    assert got == vals, (name, nreg, path, a,
                                         [(k, hex(g), hex(w)) for k, (g, w) in
                                          enumerate(zip(got, vals)) if g != w][:4])
                    assert bool(roots[a]) == bit, (name, nreg, path, a)
        finally:
            if handle is not None:
                engine.jit_detach(handle)


def test_most_folded_bench_units_generated():
    from mythril_amd.procmap import process_map
    units = list(T.MOST_FOLDED)     # (pinned there, against every C2 unit's count)
    oracle = process_map(G.oracle_root_bits, [("c2", d, FIRST, N_LANES) for d in units], 8, "spawn")
    for nreg in (11, 16):
        engine = get_engine(0, nreg=nreg)
        rows = {}
        for on in (True, False):
            progs = [(d, compile_native(bench.workload_roots("c2", d), nreg=nreg, simplify=on,
                                        leaf_remat="scratch2")) for d in units]
            assert all((p.stats["folded"] > 0) == on for _, p in progs)
            # the oracle's bits are this program's while it reads the same
            # leaves and the same constant pool
            assert all(G.oracle_inputs(p) == inp for (_, p), (_, inp) in zip(progs, oracle))
            image = jit.compile_batch([(p, None, d) for d, p in progs], workers=8, start="spawn",
                                      lds_slots=LAYOUT_LDS_SLOTS[nreg])
            for im in (None, image):
                bits, firsts = G.run_batch(engine, progs, bench.SEED, FIRST, N_LANES, im)
                G.assert_matches_oracle(bits, firsts, [w for w, _ in oracle], FIRST,
                                        ("c2", nreg, on, im is not None), units)
                rows[(on, im is not None)] = (np.asarray(bits), list(firsts))
        for compiled in (False, True):
            assert np.array_equal(rows[(True, compiled)][0], rows[(False, compiled)][0])
            assert rows[(True, compiled)][1] == rows[(False, compiled)][1]

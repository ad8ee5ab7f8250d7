"""Value parity of bench programs on the GPU: every node value and every root
bit against ``oracle/evalref.c``, not the AND of the roots.

``tests/test_gpu_bench_parity.py`` covers the whole bench configuration but
compares one bit per lane, the AND of ~47 roots, which is false on almost
every lane: a wrong 256-bit value (a spill / reload handler of the four-wave
layout, a division fast path, a narrow-spill variant) hides behind any other
false conjunct.  Here the units of ``value_units.UNITS`` — a cover of every
(family, variant) handler the bench configuration executes
(tests/test_value_units.py asserts it) plus a spread — run in three forms
compiled as the bench compiles them (``value_units.Forms``): every non-root
node probed, every root probed, and one program per root through
``batch_eval_gen`` (root bits and first satisfying indices).  Both register
layouts, interpreter and compiled programs, C2 / C3 / C4 / C5;
``value_units.check_values`` says what is compared.
"""

import contextlib
import time

import pytest

import value_units as V
from gpu_batch import run_loaded
from mythril_amd import jit
from mythril_amd.build import LAYOUT_LDS_SLOTS
from mythril_amd.engine import default_leafgen, get_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _oracle_values_shared_by_the_cases():
    """The oracle's values of a unit are computed by the first case that
    runs it and reused by the other layout and path (the leaves are the
    same); dropped after the module (about a gigabyte)."""
    yield
    V._REFS.clear()
    V._ONEROOT.clear()


class GpuExecutor:
    """The context of one register layout (as test_both_layouts_in_one_process
    makes them); ``compiled``: the programs run their compiled code
    (``jit.compile_batch`` for the layout's LDS regions), else the
    interpreter."""

    def __init__(self, nreg, compiled):
        self.engine = get_engine(0, nreg=nreg)
        self.lds = LAYOUT_LDS_SLOTS[nreg]
        assert (self.engine.nreg, self.engine.lds_slots) == (nreg, self.lds)
        self.compiled = compiled
        self.loaded = {}

    @contextlib.contextmanager
    def session(self, items):
        eng = self.engine
        loaded = [eng.load(p, default_leafgen(p), prog_seed=d) for d, p in items]
        handle = None
        if self.compiled:
            image = jit.compile_batch([(p, None, d) for d, p in items], workers=16, start="spawn",
                                      lds_slots=self.lds)
            handle = eng.jit_attach(loaded, image)
        self.loaded = {id(p): lp for (_, p), lp in zip(items, loaded)}
        try:
            yield
        finally:
            self.loaded = {}
            if handle is not None:
                eng.jit_detach(handle)

    def probed(self, items, first, n):
        return [self.engine.eval_gen(self.loaded[id(p)], V.SEED, first, n, want_probes=True,
                                     want_leaves=True) for _, p in items]

    def batch(self, items, first, n):
        return run_loaded(self.engine, [self.loaded[id(p)] for _, p in items], V.SEED, first, n)


@pytest.mark.parametrize("workload", V.WORKLOADS)
@pytest.mark.parametrize("path", ["interp", "jit"])
@pytest.mark.parametrize("nreg", [16, 11])
def test_every_node_and_root_value(nreg, path, workload):
    assert V.N_LANES % 64 == 0
    t0 = time.time()
    stats = V.check_values(GpuExecutor(nreg, path == "jit"), workload, nreg, path,
                           V.units_of(nreg, workload))
    print("%s %d-slot %s: %d units, %d nodes compared, %d roots compared, %d roots with mixed "
          "lanes, %d lanes each, %.1f s" % (workload, nreg, path, stats["units"], stats["nodes"],
                                           stats["roots"], stats["mixed"], V.N_LANES,
                                           time.time() - t0))
    assert stats["units"] == len(V.units_of(nreg, workload)) >= (32 if workload == "c2" else 8)
    assert stats["nodes"] > 0 and stats["roots"] > 0
    assert stats["mixed"] > 0, "no root of %s is true on some lanes and false on others" % workload

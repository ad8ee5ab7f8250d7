"""The full-width-divisor division path (asmgen._udivrem_full) on the GPU.

* The one-division programs of tests/div_fullwidth_cases.py (UDIV, UREM, SDIV,
  SREM, SMOD; 256 host-given lanes = the four waves (a)-(d)) through
  ``Engine.eval`` on both register layouts, interpreter and compiled code,
  every lane and limb against oracle/smtlib_ref.py.  Which path a wave takes
  is asserted on the simulator (tests/test_div_fullwidth.py); the text is the
  same.
* The eight C2 bench units with the most division records (24 to 26 of about
  430; ranked over all 4096 units by the UDIV .. SMOD counts of
  ``Program.stats["hist"]``, ties to the lower unit; tests/test_div_fullwidth.py
  checks their counts) at 1024 generated lanes:
  every node value and every root bit against oracle/evalref.c
  (``value_units.check_values``, forms nodes and rootprobe).
"""

import pytest

import div_fullwidth_cases as C
import value_units as V
from mythril_amd import jit
from mythril_amd.assign import Assignment as PA, pack
from mythril_amd.build import LAYOUT_LDS_SLOTS
from mythril_amd.engine import get_engine, limbs_to_int
from mythril_amd.ir import compile_constraints
from test_gpu_value_parity import GpuExecutor

pytestmark = pytest.mark.gpu

WAVES = ("a", "b", "c", "d")
DIVISION_UNITS = [1807, 530, 815, 1085, 2911, 3310, 1287, 2848]


@pytest.mark.parametrize("path", ["interp", "jit"])
@pytest.mark.parametrize("nreg", [16, 11])
def test_four_wave_division_programs(nreg, path):
    eng = get_engine(0, nreg=nreg)
    progs = [compile_constraints([], [C.program_nodes(op)[2]], nreg=nreg) for op in C.OPS]
    loaded = [eng.load(p) for p in progs]
    handle = None
    if path == "jit":
        image = jit.compile_batch([(p, None, 0) for p in progs], workers=1,
                                  lds_slots=LAYOUT_LDS_SLOTS[nreg])
        handle = eng.jit_attach(loaded, image)
    try:
        for op, prog, lp in zip(C.OPS, progs, loaded):
            ws = C.waves(op)
            vals = [xy for name in WAVES for xy in ws[name]]
            want = [w for name in WAVES for w in C.expected(op, name)]
            assert len(vals) == 256
            _, pr = eng.eval(lp, pack(prog, [PA(vars={"x": x, "y": y}) for x, y in vals]),
                             want_probes=True)
            got = [limbs_to_int(pr[0, :, lane]) for lane in range(256)]
            bad = [lane for lane in range(256) if got[lane] != want[lane]]
            assert not bad, "%s %d-slot %s: wave (%s) lane %d: %#x / %#x gives %#x, want %#x (%d " \
                "lanes differ)" % (op, nreg, path, WAVES[bad[0] // 64], bad[0] % 64, vals[bad[0]][0],
                                   vals[bad[0]][1], got[bad[0]], want[bad[0]], len(bad))
    finally:
        if handle is not None:
            eng.jit_detach(handle)


@pytest.mark.parametrize("path", ["interp", "jit"])
@pytest.mark.parametrize("nreg", [16, 11])
def test_division_heavy_units_every_node_and_root(nreg, path):
    stats = V.check_values(GpuExecutor(nreg, path == "jit"), "c2", nreg, path, DIVISION_UNITS,
                           forms=("nodes", "rootprobe"))
    assert stats["units"] == len(DIVISION_UNITS) and stats["nodes"] > 0 and stats["roots"] > 0

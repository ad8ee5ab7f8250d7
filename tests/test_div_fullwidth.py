"""The full-width-divisor division path (asmgen._udivrem_full) on the assembly
simulator: a wave whose every divisor keeps a nonzero top limb divides
without normalising its operands.  One division per program, the four waves
of tests/div_fullwidth_cases.py, both register layouts, the interpreter and
the compiled text, every lane and limb against oracle/smtlib_ref.py; and by
label, wave (a) never enters the general path (limb barrels and bit shifts),
waves (b) and (c) do."""

import pytest

import asm_sim
import div_fullwidth_cases as C
from mythril_amd import asmgen
from mythril_amd.assign import Assignment as PA, pack
from mythril_amd.build import LAYOUT_LDS_SLOTS
from mythril_amd.engine import limbs_to_int
from mythril_amd.ir import compile_constraints
from test_asm_sim import _max_qhat_error


@pytest.fixture
def seen(monkeypatch):
    """The instruction indices the simulated waves execute."""
    pcs = set()
    step = asm_sim.Wave.step

    def traced(self, op, a, pc):
        pcs.add(pc)
        return step(self, op, a, pc)
    monkeypatch.setattr(asm_sim.Wave, "step", traced)
    return pcs


_TEXT = {}          # the simulator's cached text per layout


@pytest.fixture
def layout(request, monkeypatch):
    """The simulator on the requested register layout (its operand table and
    its cached text belong to one layout)."""
    with asmgen.layout(request.param):
        monkeypatch.setattr(asm_sim, "OPERANDS", asm_sim._operands())
        monkeypatch.setattr(asm_sim, "_CACHE", _TEXT.setdefault(request.param, {}))
        yield request.param


def _regions(w):
    """(instruction indices of the general path: from udivrem's ``dgn`` label
    to its end label ``dsd``, which holds every limb-barrel stage and bit
    shift of the normalisation and of the remainder; indices of the
    full-width path's join label ``dfr``), over both udivrem instances of
    every division body in the text."""
    at = lambda stem: sorted(pc for l, pc in w.labels.items() if l.startswith(".L" + stem))
    general = set()
    for g in at("dgn"):
        general |= set(range(g, min(e for e in at("dsd") if e > g)))
    assert general and at("dfr")
    return general, set(at("dfr"))


def _run(op, name, nreg, jit, seen, rcp_noise=0.0):
    x, y, probe = C.program_nodes(op)
    prog = compile_constraints([], [probe], nreg=nreg)
    vals = C.waves(op)[name]
    seen.clear()
    _, pr, _, w = asm_sim.simulate(prog, pack(prog, [PA(vars={"x": a, "y": b}) for a, b in vals]),
                                   n_lds=LAYOUT_LDS_SLOTS[nreg], rcp_noise=rcp_noise, jit=jit)
    want = C.expected(op, name)
    for lane, (a, b) in enumerate(vals):
        got = limbs_to_int(pr[0, :, lane])
        assert got == want[lane], (op, name, lane, hex(a), hex(b), hex(got), hex(want[lane]))
    general, full = _regions(w)
    return bool(seen & general), bool(seen & full)


def test_wave_a_holds_what_it_should():
    """Every divisor magnitude of wave (a) is full-width, with top limbs 1,
    0x7fffffff, 0x80000000 and 0xffffffff among them (unsigned); dividends
    below, equal to and above the divisor; and its hard pairs reach a
    quotient estimate two too big."""
    for signed in (False, True):
        pairs = C.magnitude_pairs(signed)
        assert all(y >> 224 for _, y in pairs)
        tops = {y >> 224 for _, y in pairs}
        assert {1, 0x7FFFFFFF} <= tops and (signed or {0x80000000, 0xFFFFFFFF} <= tops)
        assert any(x < y for x, y in pairs) and any(x == y for x, y in pairs)
        assert any(x > y for x, y in pairs)
        # the second add-back (an estimate two too big) is reached by the
        # unsigned operators; a signed quotient is below 2^31: one add-back
        errs = [_max_qhat_error(x, y) for x, y in pairs[-C.N_HARD:]]
        if signed:
            assert max(errs) == 1 and errs.count(1) >= 3, errs
        else:
            assert max(errs) == 2 and errs.count(2) >= 3 and 1 in errs, errs
    for op in C.SIGNED:
        ws = C.waves(op)
        mags = [C.magnitude(y, True) for _, y in ws["a"]]
        assert all(m >> 224 for m in mags) and C.INT_MIN in mags
        assert {(x >> 255, y >> 255) for x, y in ws["a"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert {(x >> 255, y >> 255) for x, y in ws["d"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert (C.INT_MIN, C.M256) in ws["d"]
        assert C.magnitude(ws["b"][C.NARROW_LANE][1], True) >> 224 == 0
    assert C.waves("bvudiv")["b"][C.NARROW_LANE][1] >> 224 == 0
    assert C.waves("bvudiv")["c"][C.ZERO_LANE][1] == 0


@pytest.mark.parametrize("jit", [False, True], ids=["interp", "compiled"])
@pytest.mark.parametrize("layout", [16, 11], indirect=True)
@pytest.mark.parametrize("op", C.OPS)
def test_full_width_waves(op, layout, jit, seen):
    general, full = _run(op, "a", layout, jit, seen)
    assert full and not general, "wave (a) must divide on the full-width path alone"
    for name in ("b", "c"):
        general, full = _run(op, name, layout, jit, seen)
        assert general and not full, "wave (%s) must take the general path" % name
    _run(op, "d", layout, jit, seen)


@pytest.mark.parametrize("op", C.OPS)
def test_full_width_waves_with_reciprocal_noise(op, seen):
    """Wave (a) with v_rcp_f64 perturbed by up to 1e-7 relative, as in
    test_division_edges_with_reciprocal_noise."""
    general, full = _run(op, "a", asmgen.NREG, False, seen, rcp_noise=1e-7)
    assert full and not general


def test_quotient_only_division_leaves_no_stale_limbs(seen):
    """UDIV's quotient has limbs 1..7 zero on the full-width path whatever the
    result registers held: the division runs twice in one program, after a
    division whose quotient fills all eight limbs."""
    from mythril_amd.smt import node as N
    x, y, one = N.bv_var("x", 256), N.bv_var("y", 256), N.bv_num(1, 256)
    probes = [N.bv_op("bvudiv", x, one), N.bv_op("bvudiv", x, y), N.bv_op("bvurem", x, y)]
    prog = compile_constraints([], probes)
    vals = C.waves("bvudiv")["a"]
    _, pr, _, _ = asm_sim.simulate(prog, pack(prog, [PA(vars={"x": a, "y": b}) for a, b in vals]))
    for lane, (a, b) in enumerate(vals):
        got = [limbs_to_int(pr[k, :, lane]) for k in range(3)]
        assert got == [a, a // b, a % b], (lane, hex(a), hex(b))


def test_gpu_division_units_are_division_heavy():
    """The bench units tests/test_gpu_div_fullwidth.py runs hold at least 24
    division records each (the most any C2 unit has is 26)."""
    import bench
    from test_gpu_div_fullwidth import DIVISION_UNITS
    assert len(set(DIVISION_UNITS)) == 8
    for d in DIVISION_UNITS:
        hist = bench.compile_unit(("c2", d, 11))[1].stats["hist"]
        assert sum(hist.get(k, 0) for k in ("UDIV", "UREM", "SDIV", "SREM", "SMOD")) >= 24, d

"""The simplifying constructor of the eval-form lowering (``ir._Lowerer._rule``,
``Lowerer::rule`` in mg_compile.cpp).  CPU only.

* every rule is sound: brute force against ``oracle/smtlib_ref.py``,
  exhaustively at widths 1, 3 and 4 and on 2 000 random operand sets at
  widths 8, 33, 255 and 256, the constant in each operand position, and every
  rule must have fired;
* one named case per rule family, three cascades and two folding roots,
  compiled with the pass on and off with every node probed, through the IR
  executor and the assembly simulator (interpreter and compiled text, 16 and
  11 slots) on 64 lanes of planted leaves: on == off == ``oracle/evalref``;
* the native compiler emits what the Python specification emits, knob on and
  off;
* the candidate stream does not move: leaves, ``const_values`` and the
  default generator are equal on and off for every C2 unit and 32 units of
  each stream;
* ``MYTHRIL_GPU_SIMPLIFY=0`` gives the programs of the commit before the pass
  (pinned digests);
* the stand-alone fuzz program (tests/fuzz_simplify.cpp) runs clean under
  ASan + UBSan.
"""

import json
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bench
from mythril_amd import build, ir, irdefs as I
from mythril_amd.assign import Assignment as PA, pack
from mythril_amd.ccompile import compile_native
from mythril_amd.engine import default_leafgen, limbs_to_int
from mythril_amd.smt import node as N
from oracle import smtlib_ref as R

ROOT = build.ROOT
ONES = (1 << 256) - 1
SIGN = 1 << 255


# ----------------------------------------------------------------------------
# rule soundness by brute force
# ----------------------------------------------------------------------------

def _ref(op, w, v, imm=None):
    """The op on operand values, from the oracle's definitions."""
    m = (1 << w) - 1
    a = v[0]
    b = v[1] if len(v) > 1 else None
    if op == I.ADD:
        return (a + b) & m
    if op == I.SUB:
        return (a - b) & m
    if op == I.MUL:
        return (a * b) & m
    if op == I.NEG:
        return R.bvneg(a, w)
    if op == I.AND:
        return a & b
    if op == I.OR:
        return a | b
    if op == I.XOR:
        return a ^ b
    if op == I.NOT:
        return ~a & m
    if op == I.SHL:
        return R.bvshl(a, b, w)
    if op == I.LSHR:
        return R.bvlshr(a, b, w)
    if op == I.ASHR:
        return R.bvashr(a, b, w)
    if op == I.UDIV:
        return R.bvudiv(a, b, w)
    if op == I.UREM:
        return R.bvurem(a, b, w)
    if op == I.SDIV:
        return R.bvsdiv(a, b, w)
    if op == I.SREM:
        return R.bvsrem(a, b, w)
    if op == I.SMOD:
        return R.bvsmod(a, b, w)
    if op == I.EQ:
        return int(a == b)
    if op == I.ULT:
        return int(a < b)
    if op == I.ULE:
        return int(a <= b)
    if op == I.SLT:
        return int(R._signed(a, w) < R._signed(b, w))
    if op == I.SLE:
        return int(R._signed(a, w) <= R._signed(b, w))
    if op == I.UMULNO:
        return int(a * b < (1 << w))
    if op == I.ITE:
        return v[1] if v[0] & 1 else v[2]
    if op == I.CONCAT:
        return ((a << imm) | b) & m
    if op == I.EXTRACT:
        return (a >> imm) & m
    if op == I.SEXT:
        return R._signed(a, imm) & m
    raise AssertionError(op)


def _value(n, env, memo):
    """Value of an LNode as built (a comparison still carries its operand
    width) under leaf values ``env``."""
    r = memo.get(n.id)
    if r is None:
        if n.op == I.LEAF:
            r = env[n.imm]
        elif n.op == I.CONST:
            r = n.imm
        else:
            r = _ref(n.op, n.width, [_value(a, env, memo) for a in n.args], n.imm)
        memo[n.id] = r
    return r


BINARY = (I.ADD, I.SUB, I.MUL, I.AND, I.OR, I.XOR, I.SHL, I.LSHR, I.ASHR, I.UDIV, I.UREM, I.SDIV,
          I.SREM, I.SMOD, I.EQ, I.ULT, I.ULE, I.SLT, I.SLE, I.UMULNO)


class _Bench:
    """One lowerer with the rules on and two leaves per width."""

    def __init__(self):
        self.lw = ir._Lowerer({}, 2)
        self.lw.simplify = True
        self.checked = 0

    def leaves(self, w):
        return (self.lw.leaf("x%d" % w, w, "var", "x"), self.lw.leaf("y%d" % w, w, "var", "y"))

    def check(self, op, w, args, vals, imm=None):
        """``mk`` of ``args`` (LNodes) whose values are ``vals``."""
        n = self.lw.mk(op, w, tuple(args), imm)
        env = {}
        for a, v in zip(args, vals):
            if a.op == I.LEAF:
                env[a.imm] = v
        got, want = _value(n, env, {}), _ref(op, w, list(vals), imm)
        assert got == want, (I.OPNAME[op], w, [repr(a) for a in args], [hex(v) for v in vals],
                             hex(got), hex(want))
        self.checked += 1

    def operand_sets(self, w, a, b):
        """Every operand shape of a binary op at values a, b."""
        x, y = self.leaves(w)
        K = self.lw.const
        for op in BINARY:
            self.check(op, w, (x, y), (a, b))
            self.check(op, w, (K(a, w), y), (a, b))
            self.check(op, w, (x, K(b, w)), (a, b))
            self.check(op, w, (K(a, w), K(b, w)), (a, b))
            if a == b:
                self.check(op, w, (x, x), (a, a))
        for op in (I.NEG, I.NOT):
            self.check(op, w, (K(a, w),), (a,))
            self.check(op, w, (x,), (a,))
        # ITE: a constant, leaf or equal-armed choice
        c1 = self.lw.leaf("c", 1, "var", "c")
        for cv in (0, 1):
            self.check(I.ITE, w, (K(cv, 1), x, y), (cv, a, b))
            self.check(I.ITE, w, (K(cv, 1), K(a, w), K(b, w)), (cv, a, b))
            self.check(I.ITE, w, (c1, x, x), (cv, a, a))
            self.check(I.ITE, w, (c1, x, K(b, w)), (cv, a, b))
        # bit-field ops on constants (and on a leaf: no rule, same value)
        lo = b % w
        self.check(I.EXTRACT, w - lo, (K(a, w),), (a,), lo)
        self.check(I.EXTRACT, w - lo, (x,), (a,), lo)
        if 2 * w <= 256:
            self.check(I.CONCAT, 2 * w, (K(a, w), K(b, w)), (a, b), w)
            self.check(I.CONCAT, 2 * w, (x, K(b, w)), (a, b), w)
            self.check(I.SEXT, 2 * w, (K(a, w),), (a,), w)
        if w > 1:
            self.check(I.SEXT, w, (K(a & ((1 << lo) - 1 if lo else 1), w),),
                       (a & ((1 << lo) - 1 if lo else 1),), lo or 1)


def _special(rng, w):
    m = (1 << w) - 1
    k = rng.randrange(w)
    return rng.choice((0, 1, m, 1 << (w - 1), 1 << k, (1 << (k + 1)) - 1, rng.getrandbits(w),
                       rng.getrandbits(max(1, w // 4))))


def test_rules_sound_by_brute_force():
    b = _Bench()
    for w in (1, 3, 4):
        for x in range(1 << w):
            for y in range(1 << w):
                b.operand_sets(w, x, y)
    rng = random.Random(0x51)
    for w in (8, 33, 255, 256):
        m = (1 << w) - 1
        sets = [(x, y) for x in (0, 1, m, 1 << (w - 1)) for y in (0, 1, m, 1 << (w - 1))]
        while len(sets) < 2000:
            x = _special(rng, w)
            sets.append((x, x if rng.randrange(8) == 0 else _special(rng, w)))
        for x, y in sets:
            b.operand_sets(w, x, y)
    never = [r for r in ir.SIMPLIFY_RULES if not b.lw.fired.get(r)]
    assert never == [], never
    assert set(b.lw.fired) <= set(ir.SIMPLIFY_RULES), set(b.lw.fired) - set(ir.SIMPLIFY_RULES)
    assert b.lw.folded >= sum(b.lw.fired.values()) > 0
    print("%d constructor calls checked, %d answered by a rule" % (b.checked, b.lw.folded))


def test_const_eval_is_the_oracle():
    """The folding arithmetic itself (``ir.const_eval``; the native compiler's
    is compared through the programs below)."""
    rng = random.Random(7)
    for w in (1, 2, 8, 64, 255, 256):
        for _ in range(300):
            a, b = _special(rng, w), _special(rng, w)
            for op in BINARY:
                assert ir.const_eval(op, w, [a, b], None) == _ref(op, w, [a, b]), (op, w, a, b)


# ----------------------------------------------------------------------------
# named cases: one per rule family, cascades, folding roots
# ----------------------------------------------------------------------------

def rule_cases():
    """name -> (constraints, probes): every non-leaf node is a probe."""
    W = 256
    x, y, z = N.bv_var("x", W), N.bv_var("y", W), N.bv_var("z", W)
    c = N.bool_var("c")
    num = lambda v: N.bv_num(v & ONES, W)  # noqa: E731
    B, C = N.bv_op, N.bv_cmp
    zero, one, ones = num(0), num(1), num(ONES)
    k1, k2 = num(0x1234567890ABCDEF << 100 | 77), num(SIGN | 12345)
    arith = ("bvadd", "bvsub", "bvmul", "bvand", "bvor", "bvxor", "bvudiv", "bvurem", "bvsdiv",
             "bvsrem", "bvsmod", "bvshl", "bvlshr", "bvashr")
    cmps = ("bvult", "bvule", "bvslt", "bvsle", "bvugt", "bvsge", "bvumul_noovfl")
    cases = {}
    # -- all operands numerals (one root stays symbolic)
    vals = [B(o, k1, k2) for o in arith] + [B(o, k2, k1) for o in arith[6:]] + \
           [B("bvneg", k1), B("bvnot", k2), B("bvudiv", k1, zero), B("bvsrem", k2, zero),
            N.extract(131, 4, k1), N.concat(N.extract(127, 0, k1), N.extract(255, 128, k2)),
            N.sign_extend(128, N.extract(255, 128, k2)), N.ite(C("bvult", k1, k2), k1, k2)]
    bools = [C(o, k1, k2) for o in cmps] + [N.eq(k1, k2), N.eq(k1, k1)]
    cases["all_const"] = ([C("bvult", x, B("bvadd", *vals[:4]))] + bools[:2], vals + bools)
    # -- the same node twice
    same = [B(o, x, x) for o in ("bvsub", "bvxor", "bvand", "bvor", "bvurem", "bvsrem", "bvsmod",
                                 "bvudiv", "bvsdiv", "bvadd", "bvmul")] + [N.ite(c, y, y)]
    same_b = [C(o, x, x) for o in ("bvult", "bvule", "bvslt", "bvsle", "bvuge", "bvsgt")] + \
             [N.eq(x, x), N.bool_op("and", c, c), N.bool_op("or", c, c), N.bool_op("xor", c, c)]
    cases["same_operand"] = ([N.eq(B("bvudiv", x, x), B("bvsdiv", y, y))], same + same_b)
    # -- one numeral: sums, masks, products
    m8, p2 = num((1 << 64) - 1), num(1 << 77)
    mul = [B("bvadd", x, zero), B("bvadd", zero, x), B("bvsub", x, zero), B("bvmul", x, zero),
           B("bvmul", one, x), B("bvmul", x, p2), B("bvmul", p2, y), B("bvmul", x, m8),
           B("bvmul", x, ones), B("bvmul", num(SIGN), x), B("bvmul", x, num(3)),
           B("bvand", x, zero), B("bvand", ones, x), B("bvor", x, zero), B("bvor", ones, x),
           B("bvxor", zero, x), B("bvmul", x, y, p2)]
    cases["one_const_arith"] = ([C("bvule", B("bvmul", x, m8), B("bvmul", y, p2))], mul)
    # -- one numeral: division and shifts (x / 0 and x / 1 reach the rules
    # through a folded operand; a numeral 2^k divisor is _by_constant's)
    z0, z1 = B("bvsub", y, y), B("bvudiv", k1, k1)
    div = [B("bvudiv", x, z0), B("bvudiv", x, z1), B("bvudiv", zero, x), B("bvsdiv", x, z1),
           B("bvsdiv", zero, x), B("bvsdiv", x, z0), B("bvurem", x, z0), B("bvurem", x, z1),
           B("bvurem", zero, x), B("bvsrem", x, z0), B("bvsrem", x, z1), B("bvsrem", zero, x),
           B("bvshl", zero, x), B("bvlshr", zero, x), B("bvashr", zero, x), B("bvshl", x, z0),
           B("bvlshr", x, z0), B("bvashr", x, z0), B("bvsmod", zero, x), B("bvsmod", x, z0)]
    cases["one_const_div"] = ([N.eq(B("bvudiv", zero, x), B("bvsdiv", zero, y))], div)
    # -- one numeral: comparisons, ite, Bool connectives
    t, f = N.bool_val(True), N.bool_val(False)
    cmp1 = [C("bvumul_noovfl", x, zero), C("bvumul_noovfl", one, x), C("bvumul_noovfl", x, num(2)),
            C("bvult", x, zero), C("bvule", zero, x), C("bvule", x, ones), C("bvugt", zero, x),
            C("bvuge", x, zero), C("bvult", zero, x), C("bvslt", x, zero),
            N.bool_op("and", c, t), N.bool_op("and", f, c), N.bool_op("or", c, f),
            N.bool_op("or", t, c), N.bool_op("not", f), N.bool_op("=>", f, c),
            N.bool_op("xor", c, f)]
    ite1 = [N.ite(t, x, y), N.ite(f, x, y), N.ite(C("bvule", zero, z), x, y)]
    cases["one_const_cmp_ite"] = ([N.bool_op("or", C("bvult", x, y), C("bvule", zero, x))],
                                  cmp1 + ite1)
    # -- cascades: a fold feeding a multiply, a division, an ite
    g0 = B("bvsub", x, x)
    casc_mul = [B("bvmul", y, g0), B("bvadd", z, B("bvmul", y, g0)),
                B("bvmul", B("bvmul", y, B("bvudiv", k1, k1)), z)]
    cases["cascade_mul"] = ([C("bvult", casc_mul[1], casc_mul[2])], casc_mul)
    casc_div = [B("bvudiv", y, B("bvxor", x, x)), B("bvudiv", g0, y), B("bvurem", z, B("bvand", x, g0)),
                B("bvsdiv", B("bvudiv", y, B("bvxor", x, x)), B("bvudiv", y, B("bvxor", x, x)))]
    cases["cascade_div"] = ([N.eq(casc_div[1], casc_div[3])], casc_div)
    casc_ite = [N.ite(C("bvule", x, x), y, z), N.ite(C("bvult", g0, zero), y, B("bvmul", z, z)),
                N.ite(N.eq(B("bvurem", y, y), zero), B("bvadd", x, y), B("bvudiv", x, y))]
    cases["cascade_ite"] = ([C("bvult", casc_ite[0], casc_ite[2])], casc_ite)
    # -- roots that fold: the others and the probes are still evaluated
    cases["root_true"] = ([C("bvule", x, x), C("bvult", x, y), N.eq(y, y)], [B("bvmul", x, y)])
    cases["root_false"] = ([C("bvult", x, y), C("bvult", x, x), N.eq(x, z)], [B("bvmul", x, y)])
    out = {}
    for name, (cons, probes) in cases.items():
        every = [n for n in N.topo_order(list(cons) + list(probes))
                 if n.op not in ("var", "bvnum", "true", "false")]
        out[name] = (cons, every)
    return out


CASES = rule_cases()
PLANT = (0, 1, ONES, SIGN)


def assignments(n=64, seed=5):
    """``n`` lanes of x, y, z, c: 0, 1, ones and 2^255 in every pairing of
    x and y, then mixed widths."""
    rng = random.Random(seed)
    out = [{"x": a, "y": b, "z": rng.choice(PLANT), "c": rng.randrange(2)}
           for a in PLANT for b in PLANT]
    while len(out) < n:
        v = {k: rng.choice(PLANT) if rng.randrange(4) == 0 else
             rng.getrandbits(rng.choice((8, 64, 200, 256))) for k in "xyz"}
        if rng.randrange(4) == 0:
            v["y"] = v["x"]
        v["c"] = rng.randrange(2)
        out.append(v)
    return out[:n]


def compiled(name, nreg, on, native=True):
    cons, probes = CASES[name]
    fn = compile_native if native else ir.compile_constraints_py
    return fn(cons, probes, nreg=nreg, simplify=on)


def table_values(prog):
    return [sum(int(prog.consts[i, j]) << (32 * j) for j in range(8))
            for i in range(prog.consts.shape[0])]


_WANT = {}


def expected(name, asgs):
    """(root bit, probe values) per lane from oracle/evalref (the C oracle;
    its inputs are the source DAG and the leaf buffer, not the program)."""
    key = (name, len(asgs))
    if key not in _WANT:
        from oracle import evalref
        cons, probes = CASES[name]
        prog = compiled(name, 16, False)
        soa = pack(prog, [PA(vars=a) for a in asgs])
        S = evalref.serialize(cons, prog, probes)
        bits, vals = evalref.run_nodes_soa(S, prog, soa, [S.node_index[p.id] for p in probes])
        _WANT[key] = [(bool(bits[a]), [evalref.node_value(vals, a, k) for k in range(len(probes))])
                      for a in range(len(asgs))]
    return _WANT[key]


def test_oracle_of_the_cases_is_smtlib_ref():
    """The C oracle the cases are compared with agrees with smtlib_ref."""
    asgs = assignments(16)
    for name, (cons, probes) in CASES.items():
        for a, (bit, vals) in zip(asgs, expected(name, assignments())[:16]):
            ra = R.Assignment(vars=a)
            assert vals == [int(v) for v in R.evaluate(list(probes), ra)], name
            assert bit == bool(R.eval_constraints(cons, ra)), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_ir_executor(name):
    """The compiled records on Python integers (tests/ir_sim.py), both
    compilers' programs being equal (below): on == off == oracle."""
    import ir_sim
    asgs = assignments()
    want = expected(name, asgs)
    folded = 0
    for nreg in (16, 11):
        for on in (True, False):
            prog = compiled(name, nreg, on)
            folded += prog.stats["folded"]
            assert (prog.appended == 0 and prog.stats["folded"] == 0) or on
            assert prog.appended == 0 or prog.const_values[len(prog.const_values)] == \
                table_values(prog)[len(prog.const_values)]
            li = prog.leaf_index()
            for a, (bit, vals) in zip(asgs, want):
                lv = [0] * len(prog.leaves)
                for k, v in a.items():
                    if k in li:
                        lv[li[k]] = v
                root, pr = ir_sim.run(prog, lv)
                assert pr == vals and bool(root) == bit, (name, nreg, on, a)
    assert folded > 0, name


def sim_cases(nreg, n_lds):
    """Worker (also run in a process of the 11-slot layout): the assembly
    simulator, interpreter and compiled text, on and off, every case."""
    import asm_sim
    asgs = assignments()
    for name in sorted(CASES):
        want = expected(name, asgs)
        for on in (True, False):
            prog = compiled(name, nreg, on)
            soa = pack(prog, [PA(vars=a) for a in asgs])
            for jit in (False, True):
                root, pr, _, _ = asm_sim.simulate(prog, soa, n_lds=n_lds, jit=jit)
                for a, (bit, vals) in enumerate(want):
                    got = [limbs_to_int(pr[k, :, a]) for k in range(prog.n_probes)]
                    assert got == vals and bool(root[a]) == bit, (name, nreg, on, jit, a)
    return len(CASES)


def test_cases_assembly_simulator_16_slots():
    from mythril_amd import asmgen
    from mythril_amd.build import LAYOUT_LDS_SLOTS
    assert asmgen.NREG == 16
    assert sim_cases(16, LAYOUT_LDS_SLOTS[16]) == len(CASES)


def test_cases_assembly_simulator_11_slots():
    """The simulator runs the layout its process was started for."""
    from mythril_amd.build import LAYOUT_LDS_SLOTS
    env = dict(os.environ, MYTHGPU_NREG="11")
    env.pop("MYTHGPU_LDS_SLOTS", None)
    code = ("import sys\nsys.path.insert(0, %r)\nimport test_simplify as T\n"
            "print('cases', T.sim_cases(11, %d))\n" % (os.path.join(ROOT, "tests"),
                                                       LAYOUT_LDS_SLOTS[11]))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "cases %d" % len(CASES)


# ----------------------------------------------------------------------------
# native == Python specification
# ----------------------------------------------------------------------------

def _same(a, b):
    assert np.array_equal(a.code, b.code)
    assert np.array_equal(a.consts, b.consts)
    for f in ("const_values", "n_lds", "n_probes", "n_roots", "table_sizes", "table_kinds",
              "table_ckeys", "pool_ranges", "n_user_probes", "stats", "appended"):
        assert getattr(a, f) == getattr(b, f), f
    assert a.leaves == b.leaves


def _both(cons, probes=(), **kw):
    out = []
    for on in (True, False):
        a = ir.compile_constraints_py(cons, probes, simplify=on, **kw)
        b = compile_native(cons, probes, simplify=on, **kw)
        _same(a, b)
        out.append(b)
    return out


def test_native_is_the_specification_named_cases():
    for name, (cons, probes) in CASES.items():
        for nreg in (16, 11):
            on, off = _both(cons, probes, nreg=nreg)
            assert on.stats["folded"] > 0 and off.stats["folded"] == 0, name
        _both(cons, probes, leaf_pools=True, const_keys=True)


def test_native_is_the_specification_bench_units():
    folded = 0
    for d in range(0, 4096, 64):
        on, _ = _both(bench.workload_roots("c2", d), nreg=11)
        folded += on.stats["folded"]
    assert folded > 0
    for wl in ("c3", "c4", "c5"):
        for d in range(4):
            _both(bench.workload_roots(wl, d))


def test_programs_without_heavy_arithmetic_keep_the_plain_lowering():
    """``ir.SIMPLIFY_MIN_HEAVY``: the query streams' units (store chains over
    constant keys, no multiply or division) compile as with the pass off."""
    for wl in ("c3", "c4", "c5"):
        for d in range(0, 64, 8):
            roots = bench.workload_roots(wl, d)
            on, off = (compile_native(roots, simplify=s) for s in (True, False))
            assert on.stats["folded"] == 0 and on.appended == 0, (wl, d)
            assert np.array_equal(on.code, off.code) and np.array_equal(on.consts, off.consts)
    x, y = N.bv_var("x", 256), N.bv_var("y", 256)
    light = [N.bv_cmp("bvult", N.bv_op("bvsub", x, x), y)]
    assert compile_native(light, simplify=True).stats["folded"] == 0
    assert compile_native(light + [N.eq(N.bv_op("bvmul", x, y), y)],
                          simplify=True).stats["folded"] > 0


def test_every_constraint_keeps_a_root_record():
    """Roots that fold to one constant are not merged: ROOT records plus
    ROOT-fused producers equal the constraints, pass on and off."""
    cons, probes = CASES["root_true"]
    for nreg in (16, 11):
        for on in (True, False):
            for prog in (compiled("root_true", nreg, on), compiled("root_true", nreg, on, False)):
                ops = prog.code[:, 0] & 0xFF
                fused = (prog.code[:, 0] & I.ROOT_FLAG) != 0
                assert int((ops == I.ROOT).sum() + fused.sum()) == len(cons) == prog.n_roots


def test_unread_leaves_are_still_generated():
    """A leaf whose readers all folded away keeps a LEAF record (the last
    ones of the program): a launch that writes the leaves back writes the
    whole candidate."""
    unread = 0
    for d in range(0, 4096, 128):
        prog = compile_native(bench.workload_roots("c2", d), nreg=11, simplify=True)
        op = prog.code[:, 0] & 0xFF
        read = [int(i) for i in prog.code[op == I.LEAF][:, 2]]
        assert sorted(set(read)) == list(range(len(prog.leaves))), d
        tail = 0
        while tail < len(op) and op[len(op) - 1 - tail] == I.LEAF:
            tail += 1
        unread += tail
    assert unread > 0


def test_knob_reaches_both_compilers(monkeypatch):
    cons, probes = CASES["cascade_mul"]
    for value in (True, False):
        monkeypatch.setattr(ir, "SIMPLIFY", value)
        for comp in ("native", "py"):
            monkeypatch.setattr(ir, "COMPILER", comp)
            p = ir.compile_constraints(cons, probes)
            assert (p.stats["folded"] > 0) == value, (value, comp)
    # search-form programs keep their own folding
    monkeypatch.setattr(ir, "SIMPLIFY", True)
    monkeypatch.setattr(ir, "COMPILER", "native")
    a = ir.compile_constraints(cons, (), solve=True, leaf_pools=True, const_keys=True)
    monkeypatch.setattr(ir, "SIMPLIFY", False)
    b = ir.compile_constraints(cons, (), solve=True, leaf_pools=True, const_keys=True)
    assert a.stats["folded"] == 0 and np.array_equal(a.code, b.code)


# ----------------------------------------------------------------------------
# the candidate stream does not move
# ----------------------------------------------------------------------------

def _stream_key(item):
    """Worker: what feeds the device generator, pass on and off."""
    workload, unit = item
    roots = bench.workload_roots(workload, unit)
    out = []
    for on in (True, False):
        p = compile_native(roots, nreg=11 if workload == "c2" else 16, simplify=on)
        gens = [tuple(getattr(g, f) for f, _ in g._fields_) for g in default_leafgen(p)]
        out.append(([(l.name, l.width, l.kind, l.source, l.chunk, l.entry) for l in p.leaves],
                    list(p.const_values), gens, p.stats["folded"], p.appended,
                    table_values(p)[:len(p.const_values)] == list(p.const_values)))
    return out


# the 8 C2 units whose programs fold most (ties: the lower unit), which
# tests/test_gpu_simplify.py runs on the GPU
MOST_FOLDED = (759, 1387, 1912, 1981, 2705, 3423, 3451, 3494)


def test_candidate_stream_invariant():
    from mythril_amd.procmap import process_map
    items = [("c2", d) for d in range(bench.default_units("c2"))] + \
            [(w, d) for w in ("c3", "c4", "c5") for d in range(32)]
    folded = appended = 0
    by_unit = []
    for item, (on, off) in zip(items, process_map(_stream_key, items, min(16, os.cpu_count() or 1),
                                                  "spawn", chunksize=64)):
        assert on[:3] == off[:3], item
        assert on[5] and off[5] and off[3] == off[4] == 0, item
        folded += on[3]
        appended += on[4]
        if item[0] == "c2":
            by_unit.append((-on[3], item[1]))
    assert folded > 0 and appended > 0
    assert tuple(sorted(d for _, d in sorted(by_unit)[:8])) == MOST_FOLDED
    print("%d units: %d constructor calls folded, %d appended constant rows"
          % (len(items), folded, appended))


def test_generated_leaves_equal_on_and_off():
    from oracle import gen_ref
    for d in range(0, 4096, 64):
        roots = bench.workload_roots("c2", d)
        on, off = (compile_native(roots, nreg=11, simplify=s) for s in (True, False))
        for lane in range(4):
            idx = (3 << 20) + 192 + lane
            a = [gen_ref.gen_leaf(bench.SEED, d, li, idx, l.width, on.const_values)
                 for li, l in enumerate(on.leaves)]
            b = [gen_ref.gen_leaf(bench.SEED, d, li, idx, l.width, off.const_values)
                 for li, l in enumerate(off.leaves)]
            assert a == b, (d, lane)


# ----------------------------------------------------------------------------
# MYTHRIL_GPU_SIMPLIFY=0: the programs of the commit before the pass
# ----------------------------------------------------------------------------

# sha256(code bytes + constant table bytes) of bench.compile_unit(("c2", d, 11))
# at the parent commit
PARENT_SHA256 = {
    0: "ad7fcf53009a4000615fccfae0a1c223cd9aadff89a6b9db12d92425f10c6dda",
    256: "a824e473a0287b07ddbe380403f9e8b828e7b991bc266b1500f23e7acd486f90",
    512: "3d8bbcb18f9def0957e847381c48c7466f115b07078457b56c73f3bd6f2cd51f",
    768: "bfae851e5a9a1fd3139ac00cfbb51bfa3b2e0073c273aa1fa762e09b015a6e51",
    1024: "7d0d59c6c8aae972f35ad706293029df0a05a16ecc2cf297475af947cf415f2b",
    1280: "790480ecb160b5b18b99f017ff1d817593625dfc9cefa1b6fc5ba92d97dbbfad",
    1536: "9b1d398c5a160c2614093ea8096bbcef49c7e8284b9658410874ead6159ac5aa",
    1792: "ac8ca3ebce2624d7cda88d67320bc4690c4ad0ea8f121602b9c32ff96d8088d9",
    2048: "1c876320d7d89715fc817f80789b33a6a48c9b7c349de96ddefe80ed97e8a2d3",
    2304: "9762657c1c4b99707d19951407d308f796539f63d51c3464d95c96e6f6705b76",
    2560: "26beecb8574c566ab114fb5d63ca4d972070049d60aff24d242292feeef64a02",
    2816: "ab105950ff595136fabead3046e45e1c71bdf5beed7d46301337d99840950b82",
    3072: "da25f2e02d141a5e369d084ce1a9e9e85da74846a2ead702a60e91c071ea204f",
    3328: "64ed550805f67a43b16199aae5145ad45e0a25065581888200f41030519b742e",
    3584: "5d3eae83f7ec990147e291458a22b7427b32b3938ab9cef0294c3d02200520ab",
    3840: "e9a4dbbfa2cdb7613fbe4f5a528e0d4fac90f709341456d26c64b30e6bfea49a",
}


def test_knob_off_gives_the_parent_programs():
    code = ("import hashlib, json, bench\n"
            "out = {}\n"
            "for d in %r:\n"
            "    p = bench.compile_unit(('c2', d, 11))[1]\n"
            "    out[d] = [hashlib.sha256(p.code.tobytes() + p.consts.tobytes()).hexdigest(), "
            "p.stats['folded']]\n"
            "print(json.dumps(out))\n" % (sorted(PARENT_SHA256),))
    got = {}
    for knob in ("0", "1"):
        env = dict(os.environ, MYTHRIL_GPU_SIMPLIFY=knob)
        env.pop("MYTHRIL_GPU_COMPILER", None)
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True,
                           capture_output=True, text=True, timeout=300)
        got[knob] = json.loads(r.stdout.strip().splitlines()[-1])
    assert {int(d): v[0] for d, v in got["0"].items()} == PARENT_SHA256
    assert all(v[1] == 0 for v in got["0"].values())
    assert sum(v[1] for v in got["1"].values()) > 0
    assert sum(got["1"][d][0] != got["0"][d][0] for d in got["0"]) > 8


# ----------------------------------------------------------------------------
# roofline pricing and the stand-alone sanitizer program
# ----------------------------------------------------------------------------

def test_dag_work_prices_what_is_left(monkeypatch):
    from mythril_amd.roofline import dag_work
    x, y, z = N.bv_var("x", 256), N.bv_var("y", 256), N.bv_var("z", 256)
    B = N.bv_op
    num = lambda v: N.bv_num(v, 256)  # noqa: E731

    heavy = N.eq(B("bvsrem", y, z), x)       # (a program without heavy arithmetic keeps its price)

    def priced(node):
        monkeypatch.setattr(ir, "SIMPLIFY", True)
        on = dag_work([N.eq(node, z), heavy])
        monkeypatch.setattr(ir, "SIMPLIFY", False)
        off = dag_work([N.eq(node, z), heavy])
        assert on[0] == off[0]                       # the count does not move
        return on[1] - 528.0, off[1] - 528.0         # without the equalities and the remainder
    assert priced(B("bvsub", x, x)) == (0.0, 8.0)
    assert priced(B("bvudiv", x, x)) == (16.0, 512.0)
    assert priced(B("bvsdiv", num(0), x)) == (16.0, 512.0)
    assert priced(B("bvmul", x, num(1 << 40))) == (8.0, 192.0)
    assert priced(B("bvmul", x, num((1 << 64) - 1))) == (16.0, 192.0)
    assert priced(B("bvmul", x, num(0))) == (0.0, 192.0)
    assert priced(B("bvmul", x, y)) == (192.0, 192.0)
    assert priced(B("bvmul", x, y, num(1 << 8))) == (200.0, 384.0)
    assert priced(N.zero_extend(128, N.extract(127, 0, x))) == (16.0, 16.0)   # free before, too
    monkeypatch.setattr(ir, "SIMPLIFY", True)
    assert dag_work([N.eq(B("bvsub", x, x), z)])[1] == 16.0      # no heavy arithmetic: plain
    # a cascade: the multiply of a folded zero, and the sum that reads it
    assert priced(B("bvadd", y, B("bvmul", y, B("bvxor", x, x)))) == (0.0, 208.0)


def test_fuzz_program_under_asan_ubsan(tmp_path):
    """tests/fuzz_simplify.cpp: random small DAGs dense in equal operands and
    boundary numerals through the C ABI, a zero-initialised mgc_input (the
    pass on) — status codes, folds counted, no sanitizer report."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "fuzz_simplify")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "fuzz_simplify.cpp"),
                    os.path.join(ROOT, "mythril_amd", "csrc", "mg_compile.cpp"), "-o", exe],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "400"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    st = json.loads(r.stdout.strip().splitlines()[-1])
    assert st["dags"] == 400 and st["ok"] == 400 and st["errors"] == 0
    assert st["folded"] > 0 and st["folded_off"] == 0

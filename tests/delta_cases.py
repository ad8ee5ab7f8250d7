"""Shared by tests/test_carry_delta.py and tests/test_gpu_carry_delta.py: the
crafted groups of the delta carry, the oracle's verdict on a
whole group, and ``Engine.carry_ladder`` restated on the host."""

import numpy as np

import mythril_amd.model as M
from mythril_amd import carry as CY
from mythril_amd import engine as E
from mythril_amd.assign import Assignment
from mythril_amd.ir import Unsupported
from mythril_amd.smt import node as N
from oracle import evalref
from oracle import smtlib_ref as R

SEED = M.SEARCH_SEED


def bit(mask, l):
    return bool(int(mask[l >> 5]) >> (l & 31) & 1)


def by_leaf(prog, mask):
    return {(l.kind, l.source, l.entry) for i, l in enumerate(prog.leaves) if bit(mask, i)}


def holds(nodes, asg):
    """Every node of ``nodes`` under ``asg``, by the oracle: the list of the
    positions that fail."""
    full = R.Assignment(asg.vars, asg.arrays, asg.funcs)
    for n in N.topo_order(list(nodes)):            # model completion: a symbol the witness is
        if n.op == "var":                          # silent about is 0, an empty table
            full.vars.setdefault(n.params[0], 0)
        elif n.op in ("array", "apply") and n.params[0] not in asg.arrays and \
                n.params[0] not in asg.funcs:
            (full.arrays if n.op == "array" else full.funcs).setdefault(n.params[0], ([], 0))
    vals = R.evaluate(list(nodes), full)
    return [k for k, v in enumerate(vals) if not v]


class CpuEngine:
    """``Engine.load`` and ``Engine.carry_ladder`` on the host: the columns of
    mg_carry_fill_rungs_host (a job with fewer rungs than the batch repeats its
    last), every one evaluated by oracle/evalref on the SOURCE nodes of the job's
    program, the first true column returned as the device returns it."""

    def __init__(self):
        self.nodes, self.calls = {}, 0

    def know(self, items):
        """Remember the source nodes of the delta programs of ``items``."""
        for nodes, asg, taken in items:
            try:
                prog = CY.delta_job(nodes, asg, taken)[0]    # cached: run_delta gets the same
            except (ValueError, Unsupported):
                continue
            self.nodes[id(prog)] = (prog, CY.split_nodes(nodes, taken)[1])

    def load(self, prog, gens, prog_seed=0):
        return prog, gens, prog_seed

    def carry_ladder(self, jobs, seed, first, lanes):
        self.calls += 1
        cols = max(m.shape[0] for _, _, m in jobs) * lanes
        out = []
        for (prog, gens, prog_seed), rows, masks in jobs:
            if prog.leaves:
                soa = E.carry_fill_rungs_host(gens, prog.consts, prog_seed, rows, masks, seed,
                                              first, lanes, cols=cols)
            else:
                soa = np.zeros((0, 8, cols), dtype=np.uint32)
            src = self.nodes[id(prog)][1]
            hit = np.flatnonzero(evalref.run_leaves_soa(evalref.serialize(src, prog), prog, soa))
            if hit.size:
                c = int(hit[0])
                out.append((c, min(c // lanes, masks.shape[0] - 1), soa[:, :, c].copy()))
            else:
                out.append((-1, -1, None))
        return out


def run_delta(items, eng=None):
    eng = eng or CpuEngine()
    eng.know(items)
    return CY.run_delta(eng, items, SEED, M.search_leafgen)


def key_of(nodes):
    return M._group_key(nodes)


# ---------------------------------------------------------------------------
# a crafted parent and child
# ---------------------------------------------------------------------------

def byte(a, k):
    return N.select(a, N.bv_num(k, 256))


def calldata_group(sym_read=False):
    """(parent, new): the parent fixes calldata bytes 0..3 and bounds a var
    (with ``sym_read`` it also reads the table at that var); the child reads
    byte 4."""
    cd, v = N.array_var("dcd", 256, 8), N.bv_var("dv", 256)
    parent = [N.eq(byte(cd, k), N.bv_num(0xA0 + k, 8)) for k in range(4)]
    parent.append(N.bv_cmp("bvult", v, N.bv_num(100, 256)))
    if sym_read:
        parent.append(N.eq(N.select(cd, v), N.bv_num(0xA1, 8)))
    return parent, [N.eq(byte(cd, 4), N.bv_num(0x77, 8))]


def witness(n=6, v=1):
    """Bytes 0..3 as the parent fixes them, the rest don't-cares (byte 4 is
    0xA4, not 0x77)."""
    return Assignment(vars={"dv": v}, arrays={"dcd": ([(k, 0xA0 + k & 0xFF) for k in range(n)], 0)})


def trap():
    """select(T, x) == 1 and select(T, 3) == 1 with x == 5; the child adds
    select(T, 5) == 2: true only where x moves."""
    t, x = N.array_var("dtrap", 256, 256), N.bv_var("dtx", 256)
    one = N.bv_num(1, 256)
    parent = [N.eq(N.select(t, x), one), N.eq(N.select(t, N.bv_num(3, 256)), one)]
    new = [N.eq(N.select(t, N.bv_num(5, 256)), N.bv_num(2, 256))]
    return parent, new, Assignment(vars={"dtx": 5}, arrays={"dtrap": ([(5, 1), (3, 1)], 0)})

"""Test infrastructure of the verdict census (tests/test_census.py,
tests/test_gpu_census.py): the ladder fixture, the oracle's per-constraint
bits of a candidate range (oracle/evalref.c with its own generator), a direct
recount of the census from those bits, and the packing of bits into mask
probes."""

import functools

import numpy as np

from mythril_amd import census as CS
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N
from oracle import evalref

RS = (3, 31, 32, 33, 64, 65, 256, 257)
SEED = 0x51
PROG_SEED = 3
FIRST = (1 << 33) + 64
N_CAND = 1000


def ladder(R):
    """R constraints over three 16-bit symbols: x below R - 2 descending
    thresholds, y below 2^15, y and z distinct."""
    x, y, z = (N.bv_var(s, 16) for s in ("x", "y", "z"))
    step = 65535 // R
    roots = [N.bv_cmp("bvult", x, N.bv_num(65535 - k * step, 16)) for k in range(R - 2)]
    return roots + [N.bv_cmp("bvult", y, N.bv_num(1 << 15, 16)), N.distinct(y, z)]


@functools.lru_cache(maxsize=None)
def masked_program(key, nreg=16):
    """(constraints, eval-form program with the verdict mask as probes 0..)
    of a case: ("ladder", R) or a bench unit ("c2", 7) / ("c4", 16)."""
    if key[0] == "ladder":
        cs = ladder(key[1])
    else:
        import bench
        cs = list(bench.workload_roots(*key))
    return cs, compile_constraints(cs, CS.mask_probes(cs), nreg=nreg)


@functools.lru_cache(maxsize=None)
def oracle_bits(key, first=FIRST, n=N_CAND, seed=SEED, prog_seed=PROG_SEED):
    """(n, n_constraints) bool: every constraint on every candidate, from the
    oracle alone (the pool of the generator is the masked program's)."""
    cs, prog = masked_program(key)
    bits = evalref.run_gen(evalref.serialize(cs, prog), prog, seed, prog_seed, first, n,
                           per_root=True)
    bits.setflags(write=False)
    return bits


def recount(bits, first):
    """The census fields, counted lane by lane."""
    n, r = bits.shape
    out = {"pass": [0] * r, "first_block": [0] * r, "sole_block": [0] * r,
           "sole_index": [-1] * r, "nfail_hist": [0] * (r + 1), "best_nfail": r + 1,
           "best_index": -1, "n_roots": r, "first_index": first, "n_cand": n}
    for i in range(n):
        failing = [k for k in range(r) if not bits[i, k]]
        for k in range(r):
            out["pass"][k] += int(bits[i, k])
        out["nfail_hist"][len(failing)] += 1
        if failing:
            out["first_block"][failing[0]] += 1
        if len(failing) == 1:
            out["sole_block"][failing[0]] += 1
            if out["sole_index"][failing[0]] < 0:
                out["sole_index"][failing[0]] = first + i
        if len(failing) < out["best_nfail"]:
            out["best_nfail"], out["best_index"] = len(failing), first + i
    return out


def pack_masks(bits, n_mask=None):
    """(n, R) bool -> mask probes (n_mask, 8, n) u32 (bit k of the mask =
    column k)."""
    n, r = bits.shape
    n_mask = n_mask or CS.n_mask_probes(r)
    full = np.zeros((n, n_mask * 256), dtype=np.uint8)
    full[:, :r] = bits
    words = np.packbits(full, axis=1, bitorder="little").view("<u4")     # (n, n_mask * 8)
    return np.ascontiguousarray(words.T.reshape(n_mask, 8, n))

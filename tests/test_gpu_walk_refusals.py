"""What the repair walks refuse, word for word (mg_walk .. mg_walk_sum,
mg_walk_batch): malformed calls through the public
Engine methods on the smallest program that has a root mask, a residual probe
and a side row (`sum` of tests/sum_cases.py: no atom, no U row) at 1 walker and
16 lanes, each on every rung it applies to.  Every call is refused before
anything is uploaded or launched.  tests/golden/walk_refusals.json holds the
exception type and the full message of every call as the library and the
engine gave them before the host entries were rewritten on one mg_walk_job
(`python tests/test_gpu_walk_refusals.py --record` wrote it, on that earlier
tree); the test asserts equality case by case, so a rewrite of the host side
that changes a check's order, its rung prefix or its numbers fails here."""

import dataclasses
import functools
import json
import os
import sys

if __name__ == "__main__":                       # --record: the repository's root on the path
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

import numpy as np
import pytest

import sum_cases as SC
from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import default_leafgen, get_engine
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walk_refusals.json")
NAME = "sum"
LANES, ROUNDS = 16, 8
RUNGS = ("walk", "tree", "aim", "bound", "uf", "sum")
TREE_UP, BOUND_UP, UF_UP = RUNGS[1:], RUNGS[3:], RUNGS[4:]


@functools.lru_cache(maxsize=None)
def world():
    """The engine, the case's walk view and its full program loaded, a program
    with no leaves loaded, and the default arguments of every call."""
    eng = get_engine(0, nreg=16)
    prog = SC.program(NAME)
    gens = default_leafgen(prog)
    T = SC.trees(NAME)
    B, U, S = SC.tables(NAME)
    assert T.n_atoms == 0 and not (B.entries[:, 3] != RP.BOUND_XOR).any()   # an aim table too
    cs = [N.eq(N.bv_num(1, 8), N.bv_num(1, 8))]
    ground = compile_constraints(cs, CS.mask_probes(cs))
    assert len(ground.leaves) == 0 and ground.n_probes == 1
    w = dict(eng=eng, lp=eng.load(SC.view(NAME), gens, prog_seed=0),
             full=eng.load(prog, gens, prog_seed=0),
             ground=eng.load(ground, default_leafgen(ground), prog_seed=0))
    w["args"] = dict(lp=w["lp"], starts=SC.starts(NAME, 1), n_roots=len(SC.case(NAME)[0]),
                     table=np.array(T.roots), trees=T,
                     aims=RP.Aims(np.array(B.entries[:, :3]), B.pieces, B.sides), bounds=B, ufs=U,
                     sums=S, seed=SC.SEED, lanes=LANES, max_rounds=ROUNDS, sync_every=8,
                     mask_probe0=0, n_resid=T.n_resid)
    return w


def call(rung, a):
    """The public Engine method of ``rung`` on the arguments ``a``."""
    eng = world()["eng"]
    tail = (a["seed"], a["lanes"], a["max_rounds"], a["sync_every"], a["mask_probe0"])
    head = (a["lp"], a["starts"], a["n_roots"])
    if rung == "walk":
        return eng.walk(*head, a["table"], a["n_resid"], *tail)
    tables = {"tree": (), "aim": (a["aims"],), "bound": (a["bounds"],),
              "uf": (a["bounds"], a["ufs"]), "sum": (a["bounds"], a["ufs"], a["sums"])}[rung]
    return getattr(eng, "walk_" + rung)(*head, a["trees"], *tables, *tail, a["n_resid"])


def raw_bound_without_fixed(a):
    """mg_walk_bound with entries and a null ``fixed``: no Engine method passes
    that, so the C entry is called as ``Engine.walk_bound`` calls it."""
    import ctypes as C
    eng, T, B = world()["eng"], a["trees"], a["bounds"]
    p = lambda x: np.ascontiguousarray(x, dtype=np.uint32).ctypes.data_as(C.c_void_p)
    keep = [np.zeros((1, len(a["lp"].program.leaves), 8), np.uint32), np.zeros(1, np.uint32),
            np.zeros(1, np.uint32)]
    nr, win = C.c_uint32(), C.c_uint32()
    rc = eng.lib.mg_walk_bound(eng._ctx, a["lp"].handle, p(a["starts"]), 1, a["n_roots"], 0,
                               p(T.roots), 0, None, None, 0, a["n_resid"], p(B.entries),
                               len(B.entries), p(B.pieces), len(B.pieces), None, a["seed"],
                               LANES, ROUNDS, 8, p(keep[0]), p(keep[1]), p(keep[2]), C.byref(nr),
                               None, C.byref(win))
    eng._check(rc, "mg_walk_bound")


def _roots(k, word):
    T = world()["args"]["trees"]
    r = np.array(T.roots)
    r[k] = word
    return r


def _entry(table, col, value, row=0):
    e = np.array(table.entries)
    e[row, col] = value
    return dataclasses.replace(table, entries=e)


def _lin(k, word):
    S = world()["args"]["sums"]
    a = np.array(S.lin)
    a[k] = word
    return dataclasses.replace(S, lin=a)


def _slot_piece(a):
    """One XOR entry whose piece names slot 0 of a table with no slots."""
    return dict(bounds=RP.make_bounds([(0, [(RP.UF_SLOT | 0, 0, 0, 256)])], a["n_roots"], 0),
                sums=RP.make_sums([None], a["sums"].n_srows))


def _probe_room(a):
    """Residual probes: one more than the program has behind its root mask."""
    return a["lp"].program.n_probes - CS.n_mask_probes(a["n_roots"]) + 1


def _no_leaves(a):
    flat = RP.flat_table(1)
    none = RP.bounds_of_aims(RP.no_aims(), 1, 0)
    return dict(lp=world()["ground"], starts=np.zeros((1, 0, 8), np.uint32), n_roots=1, table=flat,
                trees=RP.simple_trees(flat), aims=RP.no_aims(), bounds=none, ufs=RP.no_ufs(),
                sums=RP.no_sums(0), n_resid=0)


# (case, the rungs it applies to, the arguments it changes)
CASES = (
    ("walkers_0", RUNGS, lambda a: dict(starts=a["starts"][:0])),
    ("walkers_65", RUNGS, lambda a: dict(starts=SC.starts(NAME, 65))),
    ("n_roots_0", RUNGS, lambda a: dict(n_roots=0)),
    ("n_roots_1025", RUNGS, lambda a: dict(n_roots=1025)),
    ("lanes_0", RUNGS, lambda a: dict(lanes=0)),
    ("max_rounds_0", RUNGS, lambda a: dict(max_rounds=0)),
    ("mask_probe0_at_n_probes", RUNGS, lambda a: dict(mask_probe0=a["lp"].program.n_probes)),
    ("n_resid_above_the_program", RUNGS, lambda a: dict(n_resid=_probe_room(a))),
    ("table_unknown_kind", ("walk",), lambda a: dict(table=_roots(1, 0xFF << 16))),
    ("table_residual_at_n_resid", ("walk",),
     lambda a: dict(table=_roots(1, RP.HAMMING << 16 | a["n_resid"]))),
    ("tree_table_malformed", TREE_UP, lambda a: dict(trees=dataclasses.replace(
        a["trees"], roots=_roots(1, RP.WT_TREE | 5)))),
    ("entry_residual_at_n_resid", ("aim",) + BOUND_UP, lambda a: dict(
        aims=_entry(a["aims"], 0, a["n_resid"]), bounds=_entry(a["bounds"], 0, a["n_resid"]))),
    ("entry_mode_5", BOUND_UP, lambda a: dict(bounds=_entry(a["bounds"], 3, 5))),
    ("slot_piece_at_n_slots", UF_UP, _slot_piece),
    ("n_urows_above_the_room", UF_UP,
     lambda a: dict(ufs=dataclasses.replace(a["ufs"], n_urows=2))),
    ("lin_unknown_word", ("sum",), lambda a: dict(sums=_lin(0, RP.SUM_NEG))),
    ("n_srows_above_the_room", ("sum",),
     lambda a: dict(sums=dataclasses.replace(a["sums"], n_srows=a["sums"].n_srows + 1))),
    ("probe_buffer_overflow", RUNGS, lambda a: dict(
        lp=world()["full"], starts=SC.starts(NAME, 64), lanes=1 << 20)),
    ("no_leaves", RUNGS, _no_leaves),
    # what the engine refuses before the library sees the call
    ("starts_shape", RUNGS, lambda a: dict(starts=a["starts"][:, :-1])),
    ("roots_shape", RUNGS, lambda a: dict(n_roots=a["n_roots"] - 1)),
    ("entries_shape", ("aim",) + BOUND_UP, lambda a: dict(
        aims=dataclasses.replace(a["aims"], entries=a["bounds"].entries),
        bounds=dataclasses.replace(a["bounds"], entries=a["aims"].entries))),
    ("fixed_shape", BOUND_UP,
     lambda a: dict(bounds=dataclasses.replace(a["bounds"], fixed=a["bounds"].fixed[:1]))),
    ("lin_shape", ("sum",),
     lambda a: dict(sums=dataclasses.replace(a["sums"], lin=a["sums"].lin[:1]))),
    ("ufs_shape", UF_UP,
     lambda a: dict(ufs=dataclasses.replace(a["ufs"], slots=np.zeros((1, 3), np.uint32)))),
)
# a batch of three jobs whose job 1 carries the case
BATCH_CASES = ("n_roots_1025", "tree_table_malformed", "entry_mode_5", "n_srows_above_the_room",
               "no_leaves")
IDS = ["%s-%s" % (name, rung) for name, rungs, _ in CASES for rung in rungs] + \
    ["bound_null_fixed-bound"] + ["%s-batch" % name for name in BATCH_CASES]


def _refusal(fn):
    eng = world()["eng"]
    ms = eng.last_kernel_ms()
    try:
        fn()
    except Exception as e:                       # the type is part of what is pinned
        assert eng.last_kernel_ms() == ms        # no launch was timed
        return {"type": type(e).__name__, "message": str(e)}
    return {"type": None, "message": "the call was not refused"}


@functools.lru_cache(maxsize=None)
def observed():
    """{id: {"type", "message"}} of every call, made once."""
    base = world()["args"]
    eng = world()["eng"]
    assert call("sum", base).rounds >= 1         # the arguments every case starts from are fine
    got = {}
    changes = {}
    for name, rungs, change in CASES:
        changes[name] = a = dict(base, **change(base))
        for rung in rungs:
            got["%s-%s" % (name, rung)] = _refusal(lambda: call(rung, a))
    got["bound_null_fixed-bound"] = _refusal(lambda: raw_bound_without_fixed(base))
    job = lambda a: (a["lp"], a["starts"], a["n_roots"], a["trees"], a["bounds"], a["ufs"],
                     a["sums"], a["seed"], a["mask_probe0"], a["n_resid"])
    for name in BATCH_CASES:
        jobs = [job(base), job(changes[name]), job(base)]
        got["%s-batch" % name] = _refusal(lambda: eng.walk_batch(jobs, LANES, ROUNDS, 8))
    assert call("sum", base).rounds >= 1         # and the context is still usable
    return got


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_these_cases():
    assert sorted(golden()) == sorted(IDS)
    assert all(v["type"] in ("EngineError", "ValueError") for v in golden().values())


@pytest.mark.parametrize("case", IDS)
def test_refusal_is_word_for_word_the_recorded_one(case):
    assert observed()[case] == golden()[case]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_walk_refusals.py --record")
    out = observed()
    assert sorted(out) == sorted(IDS)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for k in IDS:
        print(k, out[k])

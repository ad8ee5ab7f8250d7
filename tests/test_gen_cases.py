"""The conditions on the generated walk cases (tests/gen_cases.py), without a
GPU.  None is a measurement: each is asserted from the oracle
(oracle/evalref.c) and the numpy specification (mythril_amd/repair.py) alone,
at shapes of tests/test_gpu_walk_gen.py.  They say that the inputs of the GPU
parity test reach what the crafted cases do not: further root-mask and
atom-mask words and probes, waves whose lanes fail different roots and
different atoms, an OR whose minimum moves between its arms, a sum that
saturates, a descent over several rounds; that a scoring with one of seven
defects planted gives another walk on them (CATCHES names the cases); and that
the host entries of the library agree with the specification on the cases'
real masks and residuals."""

import types

import numpy as np
import pytest

import gen_cases as G
from census_cases import pack_masks
from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import default_leafgen, walk_score_host, walk_tree_score_host
from mythril_amd.ir import Unsupported
from test_walk_tree import independent_distance

LANES, WALKERS = 1000, 2              # the shape of the conditions on round 0
assert (LANES, WALKERS) in G.SHAPES
SMALL = (63, 2)                       # the shape of the planted defects
assert SMALL in G.SHAPES


def waves(lanes, walkers):
    """The columns of every run of 64 lanes of every walker (a wave of the
    score kernels: grid.y is the walker, so no wave spans two)."""
    return [np.arange(w * lanes + s, w * lanes + min(s + 64, lanes))
            for w in range(walkers) for s in range(0, lanes, 64)]


def atoms_of(T, k):
    """The atoms of tree root k, from its code."""
    out, pc = [], int(T.roots[k]) & ~RP.WT_TREE
    while int(T.code[pc]) >> 16 != RP.WT_END:
        if int(T.code[pc]) >> 16 == RP.WT_ATOM:
            out.append(int(T.code[pc]) & 0xFFFF)
        pc += 1
    return out


def tree_roots(T):
    return [k for k in range(len(T.roots)) if T.is_tree(k)]


def round0(name):
    """(failing (n, n_roots) bool, atom verdicts, residual rows) of round 0's
    neighbours at (LANES, WALKERS), from the oracle."""
    bits, abits, resid = G.round_inputs(name, WALKERS, LANES)[1]
    return ~bits, abits, resid


# ---------------------------------------------------------------------------
# limits
# ---------------------------------------------------------------------------

def test_limits_are_crossed():
    for name in ("rules", "flats"):
        assert len(G.case(name)) > 32
    assert len(G.case("rules")) % 32 == 1                   # a tail mask of one bit
    assert len(G.case("flats")) > 64 and G.trees("flats").n_atoms > 256
    assert G.trees("rules").n_atoms > 32
    for name in ("ladder_ne", "ladder_lt"):
        T = G.trees(name)
        assert len(G.case(name)) == 257 > 256 and T.is_tree(256)
        assert not any(T.is_tree(k) for k in range(256))
        kind = RP.FLAT if name == "ladder_ne" else RP.MAGNITUDE
        assert all(T.kind(k) == kind for k in range(256))
        assert CS.n_mask_probes(257) == 2
    assert G.trees("ladder_ne").n_resid == 1 and G.trees("ladder_lt").n_resid == 257
    assert G.program("ladder_lt").n_probes == 260
    # deep: the root's code, walked as the validator walks it
    T = G.trees("deep")
    assert T.is_tree(0) and tree_roots(T) == [0]
    depth = deepest = n_atom_words = 0
    pc = int(T.roots[0]) & ~RP.WT_TREE
    while int(T.code[pc]) >> 16 != RP.WT_END:
        op, arg = int(T.code[pc]) >> 16, int(T.code[pc]) & 0xFFFF
        if op in (RP.WT_ATOM, RP.WT_PUSH_INF):
            depth += 1
            n_atom_words += op == RP.WT_ATOM
        else:
            assert op in (RP.WT_AND, RP.WT_OR) and 1 <= arg <= depth
            depth -= arg - 1
        deepest = max(deepest, depth)
        pc += 1
    assert depth == 1 and deepest == RP.WT_STACK == 8
    assert n_atom_words == RP.ROOT_ATOMS == 32 == len(set(atoms_of(T, 0)))
    assert pc + 1 - (int(T.roots[0]) & ~RP.WT_TREE) == RP.ROOT_WORDS       # END included

    def nesting(s):
        return 1 if s[0] == "atom" else 1 + max(nesting(c) for c in s[1])
    assert nesting(T.shapes[0]) == RP.ROOT_DEPTH


@pytest.mark.parametrize("name", G.NAMES)
def test_every_shape_compiles_on_both_layouts(name):
    """(Where a layout refused a shape, pytest.raises(Unsupported) would stand
    here: none does.)"""
    n_roots, T = len(G.case(name)), G.trees(name)
    n_table = len(G.table_scoring(name)[0])
    for nreg in (16, 11):
        for scoring, extra in (("tree", CS.n_mask_probes(T.n_atoms) + T.n_resid),
                               ("table", n_table), ("mask", 0)):
            prog, ref = G.program(name, nreg, scoring), G.program(name, 16, scoring)
            assert prog.n_probes == CS.n_mask_probes(n_roots) + extra
            assert prog.const_values == ref.const_values
            assert [(l.source, l.width) for l in prog.leaves] == \
                [(l.source, l.width) for l in ref.leaves]
    # the census-view limit of the C ABI at the widest shape
    lanes, walkers = max(G.SHAPES, key=lambda s: s[0] * s[1])
    assert lanes * walkers * G.program(name).n_probes * 32 < 256 << 20


def test_a_second_residual_in_root_256_is_refused_on_the_11_slot_layout():
    """Why root 256 of the ladders repeats ONE equality: a change of the spill
    budget shows up here."""
    T = G.trees(G.REFUSED)
    assert len(G.case(G.REFUSED)) == 257 and T.is_tree(256) and T.n_resid == 2
    assert G.program(G.REFUSED, 16).n_probes == 2 + 1 + 2
    with pytest.raises(Unsupported, match="spill budget"):
        G.program(G.REFUSED, 11)


def test_every_walker_has_its_own_start():
    for name in G.NAMES:
        s = G.starts(name, G.MAX_WALKERS)
        assert len({r.tobytes() for r in s}) == G.MAX_WALKERS
        for i, leaf in enumerate(G.program(name).leaves):
            v = s[:, i].astype(np.uint64)
            top = sum(int(x) << (32 * j) for j, x in enumerate(np.bitwise_or.reduce(v, axis=0)))
            assert top < 1 << leaf.width and (leaf.width > 8 or top == (1 << leaf.width) - 1)
        assert np.array_equal(G.starts(name, 3), s[:3])


# ---------------------------------------------------------------------------
# round 0 of the GPU test's widest launch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", G.NAMES)
def test_waves_diverge(name):
    fail, abits, _ = round0(name)
    T = G.trees(name)
    W = waves(LANES, WALKERS)
    assert len(W) == 32
    sets = sum(len(np.unique(fail[idx], axis=0)) >= 2 for idx in W)
    assert 2 * sets >= len(W), sets                 # lanes of one wave fail different roots
    trees = tree_roots(T)
    assert name in G.TREE_CASES and trees
    mine = {k: atoms_of(T, k) for k in trees}
    split = 0
    for idx in W:
        split += any(len(np.unique(abits[idx][fail[idx, k]][:, mine[k]], axis=0)) >= 2
                     for k in trees if fail[idx, k].sum() >= 2)
    assert 2 * split >= len(W), split               # .. and one tree root by different atoms
    n_words = (len(T.roots) + 31) // 32
    assert all(fail[:, 32 * q:32 * q + 32].any() for q in range(n_words))
    false_under = np.zeros(T.n_atoms, dtype=bool)   # atoms false in a lane that fails their root
    for k in trees:
        false_under[mine[k]] |= (~abits[fail[:, k]][:, mine[k]]).any(axis=0)
    a_words = (T.n_atoms + 31) // 32
    assert all(false_under[32 * q:32 * q + 32].any() for q in range(a_words))
    assert a_words == {"rules": 2, "flats": 11}.get(name, 1)


def arm_trees(T, first):
    """``T`` with every OR replaced by its first arm (``first``) or by the OR
    of its later arms: the shapes alone, for ``independent_distance``."""
    def cut(s):
        if s[0] not in ("and", "or"):
            return s
        kids = [cut(c) for c in s[1]]
        if s[0] == "and":
            return ("and", kids)
        return kids[0] if first else kids[1] if len(kids) == 2 else ("or", kids[1:])
    return types.SimpleNamespace(roots=T.roots, atoms=T.atoms, is_tree=T.is_tree,
                                 shapes=[cut(s) for s in T.shapes])


@pytest.mark.parametrize("name", ("flats", "rules"))
def test_or_picks_both_arms(name):
    """For some root, the OR's minimum is the first arm's alone in one lane
    that fails the root and a later arm's alone in another."""
    fail, abits, resid = round0(name)
    T = G.trees(name)
    A, B = arm_trees(T, True), arm_trees(T, False)
    lanes = range(0, 256)                            # walker 0's first four waves
    vals = [[int.from_bytes(np.ascontiguousarray(resid[p, :, j]).tobytes(), "little")
             for p in range(T.n_resid)] for j in lanes]
    both = []
    for k in tree_roots(T):
        if "or" not in repr(T.shapes[k]):
            continue
        seen = set()
        for j in lanes:
            if not fail[j, k]:
                continue
            args = (k, abits[j], vals[j])
            d, a, b = (independent_distance(t, *args) for t in (T, A, B))
            assert d == min(a, b) or name == "rules"      # (rules nests an OR under an AND)
            seen.add("first" if a == d < b else "later" if b == d < a else "tie")
        if {"first", "later"} <= seen:
            both.append(k)
    assert both, name


def test_saturation_happens():
    fail, abits, resid = round0("deep")
    T = G.trees("deep")
    only = np.ones_like(fail)
    only[:, 0] = ~fail[:, 0]                         # bits: root 0 alone may fail
    value = RP._tree_score_bits(only, abits, resid, T)[1][fail[:, 0]]
    assert (value == RP.WT_INF).any() and (value < RP.WT_INF).any()
    assert fail[:, 0].sum() > LANES


@pytest.mark.parametrize("name", G.NAMES)
def test_the_walks_move(name):
    """Walker 0's trace falls strictly at least three times in the 8 rounds
    (the ladders: by the four window equalities of root 256, some 32 bits
    away at a random start and a bit or two nearer per round)."""
    assert G.rounds_at(name, (LANES, WALKERS)) == G.ROUNDS == 8
    res = G.reference(name, WALKERS, LANES)
    keys = res.trace[0, :res.rounds].astype(np.int64)
    keys = keys[:, 0] << 20 | keys[:, 1]
    assert (np.diff(keys) <= 0).all()
    falls = int((np.diff(keys) < 0).sum())
    assert falls >= 3 and res.rounds == G.ROUNDS, keys.tolist()
    if name.startswith("ladder"):              # .. and it is root 256 that descends
        assert res.trace[0, 0, 0] >= 1 and G.trees(name).is_tree(256)
        final = G.values_fn(name)(np.ascontiguousarray(res.leaves[0][:, :, None]))[0][0]
        assert res.nfail[0] == 0 or not final[256]


# ---------------------------------------------------------------------------
# planted defects
# ---------------------------------------------------------------------------

def local_score(bits, abits, resid, T, or_first=False, saturate=True):
    """A copy of repair._tree_score_bits with two switches."""
    fail = ~np.asarray(bits, dtype=bool)
    n = fail.shape[0]
    pop, length = RP._distances(resid, n) if len(resid) else (None, None)

    def dist(e):
        kind, p = int(e) >> 16, int(e) & 0xFFFF
        return (np.ones(n, dtype=np.int64) if kind == RP.FLAT else
                np.maximum(1, pop[p]) if kind == RP.HAMMING else 1 + length[p])
    cost = np.zeros(n, dtype=np.int64)
    for k in np.flatnonzero(fail.any(axis=0)):
        e = int(T.roots[k])
        if not e & RP.WT_TREE:
            cost += fail[:, k] * dist(e)
            continue
        stack, pc = [], e & ~RP.WT_TREE
        while int(T.code[pc]) >> 16 != RP.WT_END:
            op, arg = int(T.code[pc]) >> 16, int(T.code[pc]) & 0xFFFF
            pc += 1
            if op == RP.WT_ATOM:
                stack.append(np.where(abits[:, arg], 0, dist(T.atoms[arg])))
            elif op == RP.WT_PUSH_INF:
                stack.append(np.full(n, RP.WT_INF, dtype=np.int64))
            else:
                args = stack[len(stack) - arg:]
                del stack[len(stack) - arg:]
                if op == RP.WT_AND:
                    v = np.sum(args, axis=0)
                    stack.append(np.minimum(RP.WT_INF, v) if saturate else v)
                else:
                    stack.append(args[0] if or_first else np.min(args, axis=0))
        top = np.maximum(stack[0], 1)
        cost += fail[:, k] * (np.minimum(top, RP.WT_INF) if saturate else top)
    return fail.sum(axis=1).astype(np.int64), cost


DEFECTS = {
    1: "root-mask words q >= 1 ignored",
    2: "the root-mask probe beyond the first ignored",
    3: "atom bits at index 32 and beyond read as true",
    4: "atom bits at index 256 and beyond read as true",
    5: "OR takes its first arm",
    6: "no saturation, neither of a sum nor of a root's value",
    7: "a lane's failing set replaced by its wave's union",
}
# which cases' reference walks at SMALL differ under which defect
CATCHES = {
    1: ("rules", "flats", "ladder_lt"),
    2: ("ladder_ne", "ladder_lt"),
    3: ("rules", "flats"),
    4: ("flats",),
    5: ("rules", "flats"),
    6: ("deep",),
    7: G.NAMES,
}


def planted(T, defect, lanes):
    """tree_scoring(T) with ``defect`` planted (0: none)."""
    def score(bits, abits, resid):
        bits, abits = np.array(bits), np.array(abits)
        if defect == 1:
            bits[:, 32:] = True
        elif defect == 2:
            bits[:, 256:] = True
        elif defect == 3:
            abits[:, 32:] = True
        elif defect == 4:
            abits[:, 256:] = True
        elif defect == 7:
            for idx in waves(lanes, len(bits) // lanes):
                bits[idx] = bits[idx].all(axis=0)
        return local_score(bits, abits, resid, T, or_first=defect == 5, saturate=defect != 6)
    return score


def walked(name, defect):
    lanes, walkers = SMALL
    prog, T = G.program(name), G.trees(name)
    return RP.walk_ref(G.values_fn(name), default_leafgen(prog), G.consts_of(prog),
                       G.starts(name, walkers), T.roots, G.SEED, lanes, G.ROUNDS, 8,
                       score=planted(T, defect, lanes))


def differs(a, b):
    return not (np.array_equal(a.leaves, b.leaves) and np.array_equal(a.nfail, b.nfail)
                and np.array_equal(a.cost, b.cost) and np.array_equal(a.trace, b.trace))


@pytest.mark.parametrize("name", G.NAMES)
def test_the_references_see_the_planted_defects(name):
    true = G.reference(name, SMALL[1], SMALL[0])
    assert not differs(walked(name, 0), true)        # the local copy is the specification
    for defect, cases in CATCHES.items():
        if name in cases:
            assert differs(walked(name, defect), true), DEFECTS[defect]


def test_all_seven_defects_are_caught():
    assert sorted(CATCHES) == sorted(DEFECTS) == list(range(1, 8))
    assert all(cases and set(cases) <= set(G.NAMES) for cases in CATCHES.values())


# ---------------------------------------------------------------------------
# the host entries on the cases' own masks and residuals
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", G.NAMES)
def test_host_entries_equal_the_specification(name):
    bits, abits, resid = G.round_inputs(name, WALKERS, LANES)[1]
    T, n_roots = G.trees(name), len(G.case(name))
    masks, amasks = pack_masks(bits), pack_masks(abits)
    assert masks.shape[0] == CS.n_mask_probes(n_roots)
    assert amasks.shape[0] == CS.n_mask_probes(T.n_atoms)
    want = RP.tree_score_ref(masks, amasks, resid, T, n_roots)
    got = walk_tree_score_host(masks, amasks, resid, T, n_roots)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(want[0], (~bits).sum(axis=1)) and want[0].max() > 0
    assert np.array_equal(want[1], RP.tree_scoring(T)(bits, abits, resid)[1])
    tbits, tresid = G.round_inputs(name, WALKERS, LANES, "table")[1]
    table = G.table_scoring(name)[1]
    tmasks = pack_masks(tbits)
    want = RP.score_ref(tmasks, tresid, table, n_roots)
    got = walk_score_host(tmasks, tresid if len(tresid) else None, table, n_roots)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(want[0], (~tbits).sum(axis=1))

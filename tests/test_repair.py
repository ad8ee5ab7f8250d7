"""The local search without a GPU: the library's move
function (csrc/mg_repair.h through mg_repair_mutate_host) against its numpy
specification (repair.mutate_ref) in every limb, the properties of the move
set, the refusals of the host entry, and the conditions on the crafted cases
(tests/repair_cases.py): repair_ref through the oracle reaches a model within
half of the round budget where the generator finds none among lanes x
max_rounds candidates."""

import ctypes as C

import numpy as np
import pytest

import repair_cases as K
from mythril_amd import repair as RP
from mythril_amd.engine import EngineError, LeafGen, load_library, repair_mutate_host

WIDTHS = (1, 8, 31, 32, 33, 64, 255, 256)
LANES = (1, 63, 64, 65, 1000)
ROUNDS = (0, 1, (1 << 16) - 1)
SEED = 0xC0FFEE1234567


def leaf_set(n_leaves, pools):
    """(leaf table, constants, canonical random base): widths cycle through
    WIDTHS (33 leaves: 1..33); ``pools``: every other leaf draws from a pool
    of its own, the rest have none."""
    rng = np.random.default_rng(n_leaves * 2 + pools)
    widths = list(range(1, 34)) if n_leaves == 33 else [WIDTHS[-1 - i] for i in range(n_leaves)]
    if n_leaves == len(WIDTHS):
        widths = list(WIDTHS)
    consts = rng.integers(0, 1 << 32, (7, 8), dtype=np.uint32)
    consts[0] = 0                                   # pool value - 1 wraps
    consts[1] = 0xFFFFFFFF                          # pool value + 1 wraps
    gens = [LeafGen(w, i % 5, 1 + i % 3 if pools and i % 2 == 0 else 0, 0, 0, 0)
            for i, w in enumerate(widths)]
    base = rng.integers(0, 1 << 32, (n_leaves, 8), dtype=np.uint32)
    for i, w in enumerate(widths):
        v = int.from_bytes(base[i].tobytes(), "little") & ((1 << w) - 1)
        base[i] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    return gens, consts, base, widths


SETS = [(n, p) for n in (1, 2, 8, 33) for p in (0, 1)]


@pytest.mark.parametrize("n_leaves,pools", SETS)
def test_library_moves_equal_the_specification(n_leaves, pools):
    gens, consts, base, widths = leaf_set(n_leaves, pools)
    kinds = set()
    for lanes in LANES:
        for r in ROUNDS:
            want = RP.mutate_ref(gens, consts, base, SEED, r, lanes)
            got, moves = repair_mutate_host(gens, consts, base, SEED, r, lanes)
            assert got.shape == (n_leaves, 8, lanes)
            assert np.array_equal(got, want), (lanes, r, np.argwhere(got != want)[:4])
            assert np.array_equal(got[:, :, 0], base)               # lane 0 is the base
            spec = RP.moves_ref(gens, consts, base, SEED, r, lanes)
            for j, row in enumerate(spec):
                assert moves[j, 0] == len(row) == (0 if j == 0 else 1 if j < lanes // 2 else 2)
                assert [int(moves[j, 2 + m]) for m in range(len(row))] == [m[0] for m in row]
                assert [int(moves[j, 1]) >> (8 * m) & 0xFF for m in range(len(row))] == \
                    [m[1] for m in row]
                kinds.update(m[1] for m in row)
            two = np.flatnonzero(moves[:, 0] == 2)
            assert two.size == 0 or two.min() >= max(1, lanes // 2)  # two moves: upper half only
            for i, w in enumerate(widths):                           # canonical values
                top = got[i].astype(object)
                vals = sum(top[k] << (32 * k) for k in range(8))
                assert all(int(v) >> w == 0 for v in vals), (i, w)
            # a lane range is the same lanes
            if lanes == 1000:
                part, pm = repair_mutate_host(gens, consts, base, SEED, r, lanes, 448, 200)
                assert np.array_equal(part, want[:, :, 448:648])
                assert np.array_equal(pm, moves[448:648])
    assert kinds == set(range(RP.KINDS))                             # all six move kinds occur


def test_moves_change_what_they_say():
    """Every kind, on a 256-bit leaf with a pool and on one without: the
    value differs from the base only as the kind allows."""
    gens = [LeafGen(256, 2, 3, 0, 0, 0), LeafGen(64, 0, 0, 0, 0, 0)]
    _, consts, _, _ = leaf_set(2, 1)
    base = np.zeros((2, 8), dtype=np.uint32)
    base[0] = np.arange(1, 9, dtype=np.uint32) * 0x01010101
    base[1, :2] = (0xDEADBEEF, 0x12345678)
    ints = [int.from_bytes(b.tobytes(), "little") for b in base]
    cvals = [int.from_bytes(c.tobytes(), "little") for c in consts]
    seen = set()
    for j, row in enumerate(RP.moves_ref(gens, consts, base, SEED, 3, 1000)[:500]):
        for leaf, kind, v in row:                      # one-move lanes: from the base
            w, old = (256, 64)[leaf], ints[leaf]
            d = v ^ old
            if kind == RP.FLIP:
                assert bin(d).count("1") == 1
            elif kind == RP.STEP:
                diff = (v - old) % (1 << w)
                assert bin(diff).count("1") == 1 or bin((-diff) % (1 << w)).count("1") == 1
            elif kind == RP.BYTE:
                assert d == 0 or (d >> (8 * ((d.bit_length() - 1) // 8))) < 256 and \
                    d & ((1 << (8 * ((d.bit_length() - 1) // 8))) - 1) == 0
            elif kind == RP.LIMB:
                assert d == 0 or d >> (32 * ((d.bit_length() - 1) // 32)) < (1 << 32) and \
                    d & ((1 << (32 * ((d.bit_length() - 1) // 32))) - 1) == 0
            elif kind == RP.POOL and leaf == 0:
                assert any(v == (cvals[2 + e] + dl - 1) % (1 << 256)
                           for e in range(3) for dl in range(3))
            elif kind == RP.POOL:
                assert v in (0, 1, 1 << 63, (1 << 64) - 1)
            else:
                assert v in (old, ints[1 - leaf] & ((1 << w) - 1))
            seen.add((leaf, kind))
    assert seen == {(l, k) for l in range(2) for k in range(RP.KINDS)}


def test_host_entry_refusals():
    lib = load_library()
    gens, consts, base, _ = leaf_set(2, 1)
    assert repair_mutate_host(gens, consts, base, SEED, 0, 64)[0].shape == (2, 8, 64)
    bad = [dict(lanes=0), dict(lanes=(1 << 20) + 1), dict(r=1 << 16), dict(lane0=65),
           dict(lane0=10, n_lanes=55)]
    for kw in bad:
        args = dict(seed=SEED, r=0, lanes=64, lane0=0, n_lanes=None)
        args.update(kw)
        with pytest.raises(EngineError, match=r"\(-1\)"):
            repair_mutate_host(gens, consts, base, **args)
    for g in ([LeafGen(0, 0, 0, 0, 0, 0)], [LeafGen(257, 0, 0, 0, 0, 0)],
              [LeafGen(8, 6, 2, 0, 0, 0)]):                          # width, pool past the consts
        with pytest.raises(EngineError):
            repair_mutate_host(g, consts, np.zeros((1, 8), dtype=np.uint32), SEED, 0, 64)
    wide = np.zeros((1, 8), dtype=np.uint32)
    wide[0, 0] = 0x100                                               # a base beyond its width
    with pytest.raises(EngineError):
        repair_mutate_host([LeafGen(8, 0, 0, 0, 0, 0)], consts, wide, SEED, 0, 64)
    with pytest.raises(EngineError):
        repair_mutate_host([], consts, np.zeros((0, 8), dtype=np.uint32), SEED, 0, 64)
    # null pointers
    garr = (LeafGen * 2)(*gens)
    out = np.zeros((2, 8, 64), dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = [C.cast(garr, C.c_void_p), 2, p(consts), consts.shape[0], p(base), SEED, 0, 64, 0, 64,
            p(out), None]
    assert lib.mg_repair_mutate_host(*good) == 0
    for k in (0, 2, 4, 10):
        q = list(good)
        q[k] = None
        assert lib.mg_repair_mutate_host(*q) == -1


@pytest.mark.parametrize("name", K.NAMES)
def test_crafted_cases_need_the_local_search(name):
    """The conditions on the inputs: repair_ref (through the oracle) reaches
    a model within half of max_rounds from the case's start, which is not a
    model itself, and the generator finds none among lanes x max_rounds."""
    res = K.reference(name)
    bits = K.bits_fn(name)
    start = K.start_rows(name)
    assert not bits(start[:, :, None])[0].all()
    assert res.nfail == 0 and bits(np.asarray(res.leaves)[:, :, None])[0].all()
    first_zero = int(np.argmax(res.trace[:res.rounds] == 0))
    assert res.trace[first_zero] == 0 and first_zero < K.MAX_ROUNDS // 2
    assert res.rounds <= K.MAX_ROUNDS // 2 and res.rounds % 8 == 0
    assert (np.diff(res.trace[:res.rounds].astype(np.int64)) <= 0).all()       # never regresses
    assert K.generator_hits(name, K.LANES * K.MAX_ROUNDS) == 0


def test_reference_loop_stops_and_syncs_as_specified():
    """lanes = 1 returns the start with its own count after max_rounds; the
    sync interval only delays the stop."""
    name = "narrow"
    bits = K.bits_fn(name)
    start = K.start_rows(name)
    one = K.reference(name, 1, 12, 8)
    assert np.array_equal(one.leaves, start) and one.rounds == 12
    assert one.nfail == int((~bits(start[:, :, None])[0]).sum()) == 5
    assert (one.trace == one.nfail).all()
    a, b, c = (K.reference(name, 1000, 24, s) for s in (1, 8, 24))
    assert a.nfail == b.nfail == c.nfail and np.array_equal(a.leaves, b.leaves)
    assert np.array_equal(b.leaves, c.leaves) and a.rounds <= b.rounds <= c.rounds == 24
    assert np.array_equal(a.trace[:a.rounds], c.trace[:a.rounds])

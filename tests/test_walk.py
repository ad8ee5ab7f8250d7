"""The scored walk without a GPU: the residual probes
against oracle/smtlib_ref.py, the library's scoring function (csrc/mg_walk.h
through mg_walk_score_host) against its numpy specification
(repair.score_ref), walk_ref against repair_ref and against single walkers,
and the conditions on the crafted cases (tests/walk_cases.py): the generator
finds no model, the count alone (repair_ref) stays stuck, the scored walk
reaches a model within half of the round budget."""

import ctypes as C

import numpy as np
import pytest

import repair_cases as RK
import walk_cases as K
from mythril_amd import repair as RP
from mythril_amd.engine import EngineError, default_leafgen, load_library, walk_score_host
from mythril_amd.smt import node as N
from oracle import smtlib_ref as R

FLAT, HAMMING, MAGNITUDE = RP.FLAT, RP.HAMMING, RP.MAGNITUDE


def pack_masks(bits):
    """(n, n_roots) bool -> mask probes (n_mask, 8, n) u32 (bit k of the mask
    is root k)."""
    n, n_roots = bits.shape
    n_mask = (n_roots + 255) // 256
    padded = np.zeros((n, n_mask * 256), dtype=np.uint8)
    padded[:, :n_roots] = bits
    words = np.packbits(padded, axis=1, bitorder="little").view("<u4")        # (n, n_mask * 8)
    return np.ascontiguousarray(words.T.reshape(n_mask, 8, n))


def rows_of(values, n):
    """Python ints [probe][lane] -> (n_probes, 8, n) u32."""
    out = np.zeros((len(values), 8, n), dtype=np.uint32)
    for p, row in enumerate(values):
        for a, v in enumerate(row):
            out[p, :, a] = np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u4")
    return out


def shapes(rng):
    """One constraint of every row of the residual table over a few 4..16-bit
    symbols: (constraint, kind, (a, b) with R = a xor b or a - b, or None)."""
    ws = (4, 7, 8, 13, 16)
    sym = {w: [N.bv_var("s%d_%d" % (w, i), w) for i in range(3)] for w in ws}

    def term(w):
        a, b = rng.choice(3, 2, replace=False)
        pick = rng.integers(4)
        if pick == 0:
            return sym[w][a]
        if pick == 1:
            return N.bv_op("bvadd", sym[w][a], sym[w][b])
        if pick == 2:
            return N.bv_num(int(rng.integers(1 << w)), w)
        return N.bv_op("bvxor", sym[w][a], N.bv_num(int(rng.integers(1 << w)), w))

    def word(c, w=256):                      # LASER's Bool as a word
        return N.ite(c, N.bv_num(1, w), N.bv_num(0, w))

    out = []
    for w in ws:
        a, b = term(w), sym[w][int(rng.integers(3))]
        eq = N.eq(a, b)
        out.append((eq, HAMMING, (a, b)))
        out.append((N.bool_op("not", N.bool_op("not", eq)), HAMMING, (a, b)))
        out.append((N.eq(word(eq), N.bv_num(1, 256)), HAMMING, (a, b)))
        out.append((N.bool_op("not", N.eq(word(eq), N.bv_num(0, 256))), HAMMING, (a, b)))
        out.append((N.eq(word(N.bool_op("not", eq), 8), N.bv_num(0, 8)), HAMMING, (a, b)))
        out.append((N.bool_op("not", eq), FLAT, None))                      # a negated equality
        out.append((N.eq(word(eq), N.bv_num(0, 256)), FLAT, None))          # LASER's not
        for op in ("bvult", "bvule", "bvslt", "bvsle"):
            a, b = term(w), term(w)
            out.append((N.bv_cmp(op, a, b), MAGNITUDE, (a, b)))
        for op in ("bvugt", "bvuge", "bvsgt", "bvsge"):
            a, b = term(w), term(w)
            out.append((N.bv_cmp(op, a, b), MAGNITUDE, (b, a)))
        a, b = term(w), term(w)                                             # LASER's UGE
        out.append((N.bool_op("or", N.bv_cmp("bvugt", a, b), N.eq(a, b)), MAGNITUDE, (b, a)))
        out.append((N.bool_op("or", N.eq(a, b), N.bool_var("flag"), N.bv_cmp("bvsle", a, b)),
                    MAGNITUDE, (a, b)))
        out.append((N.eq(word(N.bv_cmp("bvult", a, b)), N.bv_num(1, 256)), MAGNITUDE, (a, b)))
        out.append((N.bool_op("not", N.bv_cmp("bvult", a, b)), FLAT, None))
        out.append((N.bool_op("or", N.eq(a, b), N.bool_var("flag")), FLAT, None))
        out.append((N.bool_op("and", N.eq(a, b), N.bv_cmp("bvult", a, b)), FLAT, None))
        out.append((N.distinct(a, b), FLAT, None))
    x1 = N.bv_var("bit", 1)
    out.append((N.eq(x1, N.bv_num(1, 1)), FLAT, None))                      # distance always 1
    out.append((N.bool_var("flag"), FLAT, None))
    wide = [N.bv_var("wide%d" % i, 256) for i in range(2)]
    big = N.concat(wide[0], wide[1])                                        # 512 bits
    out.append((N.eq(big, N.concat(wide[1], wide[0])), FLAT, None))
    out.append((N.bv_cmp("bvult", big, N.concat(wide[1], wide[0])), FLAT, None))
    out.append((N.eq(wide[0], wide[1]), HAMMING, (wide[0], wide[1])))
    out.append((N.bv_cmp("bvslt", wide[0], wide[1]), MAGNITUDE, (wide[0], wide[1])))
    return out


def random_assignment(nodes, rng):
    asg = {}
    for n in N.topo_order(nodes):
        if n.op == "var":
            w = 1 if n.is_bool() else n.width
            v = int.from_bytes(rng.bytes(32), "little") & ((1 << w) - 1)
            asg[n.params[0]] = v if rng.integers(4) else v & 3       # (near values: equalities hold)
    return R.Assignment(asg)


@pytest.mark.parametrize("seed", range(4))
def test_residuals_mean_what_the_table_says(seed):
    rng = np.random.default_rng(seed)
    rows = shapes(rng)
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    cs = [r[0] for r in rows]
    probes, table = RP.residuals(cs)
    assert table.shape == (len(cs),) and table.dtype == np.uint32
    assert [int(t) >> 16 for t in table] == [r[1] for r in rows]
    assert all(p.is_bv() and p.width <= 256 for p in probes)
    assert len({p.id for p in probes}) == len(probes)                       # one per term
    n = 48
    bits = np.zeros((n, len(cs)), dtype=bool)
    resid = [[0] * n for _ in probes]
    want_cost = np.zeros(n, dtype=np.int64)
    for a in range(n):
        asg = random_assignment(cs, rng)
        holds = R.evaluate(cs, asg)
        vals = R.evaluate(probes, asg) if probes else []
        for p, v in enumerate(vals):
            resid[p][a] = v
        for k, (c, kind, ab) in enumerate(rows):
            bits[a, k] = bool(holds[k])
            d = 1
            if ab is not None:
                p = int(table[k]) & 0xFFFF
                va, vb = R.evaluate(list(ab), asg)
                w = ab[0].width
                want = va ^ vb if kind == HAMMING else (va - vb) % (1 << w)
                assert vals[p] == want, (k, kind)
                d = max(1, bin(want).count("1")) if kind == HAMMING else 1 + want.bit_length()
                if kind == HAMMING:                       # the mask and the residual agree
                    assert bool(holds[k]) == (want == 0)
            else:
                assert int(table[k]) == FLAT << 16
            assert d >= 1
            if not holds[k]:
                want_cost[a] += d
    assert (~bits).any(axis=0).sum() > len(cs) // 2                         # roots do fail
    nfail, cost = RP.score_ref(pack_masks(bits), rows_of(resid, n), table, len(cs))
    assert np.array_equal(nfail, (~bits).sum(axis=1))
    assert np.array_equal(cost, want_cost) and (cost >= nfail).all()
    assert (cost[nfail > 0] >= 1).all() and not cost[nfail == 0].any()
    # every root FLAT: the cost is the count
    nf, co = RP.score_ref(pack_masks(bits), None, RP.flat_table(len(cs)), len(cs))
    assert np.array_equal(nf, nfail) and np.array_equal(co, nfail)
    # the library scores the same
    nf, co = walk_score_host(pack_masks(bits), rows_of(resid, n), table, len(cs))
    assert np.array_equal(nf, nfail) and np.array_equal(co, cost)


def score_inputs(n_roots, n, seed):
    """Random verdicts (most roots hold), a random table over residuals of
    every width 1..256 (zero and one-bit values among them)."""
    rng = np.random.default_rng(seed)
    bits = rng.random((n, n_roots)) < 0.8
    bits[0] = True
    bits[1] = False
    n_resid = min(256, max(1, n_roots))
    widths = rng.permutation(np.arange(1, 257))[:n_resid] if n_resid < 256 else np.arange(1, 257)
    resid = np.zeros((n_resid, 8, n), dtype=np.uint32)
    for p, w in enumerate(widths):
        for a in range(n):
            v = int.from_bytes(rng.bytes(32), "little") & ((1 << int(w)) - 1)
            pick = rng.integers(6)
            v = 0 if pick == 0 else 1 << int(rng.integers(w)) if pick == 1 else \
                v | 1 << (int(w) - 1) if pick == 2 else v
            resid[p, :, a] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    kind = rng.integers(0, 3, n_roots)
    probe = rng.integers(0, n_resid, n_roots)
    table = (kind << 16 | np.where(kind == FLAT, 0, probe)).astype(np.uint32)
    return bits, resid, table


@pytest.mark.parametrize("n_roots", (1, 31, 32, 33, 256, 257))
def test_library_scores_equal_the_specification(n_roots):
    n = 130
    bits, resid, table = score_inputs(n_roots, n, n_roots)
    masks = pack_masks(bits)
    # bits at or above n_roots are ignored
    junk = np.random.default_rng(1).integers(0, 1 << 32, masks.shape, dtype=np.uint32)
    valid = pack_masks(np.ones((n, n_roots), dtype=bool))
    masks = masks | (junk & ~valid)
    want_nfail, want_cost = RP.score_ref(masks, resid, table, n_roots)
    nfail, cost = walk_score_host(masks, resid, table, n_roots)
    assert np.array_equal(nfail, want_nfail) and np.array_equal(cost, want_cost)
    assert nfail[0] == 0 == cost[0] and nfail[1] == n_roots <= cost[1]
    assert set((table >> 16).tolist()) == {FLAT, HAMMING, MAGNITUDE} or n_roots == 1
    # independently, lane by lane from Python ints
    ints = [[int.from_bytes(resid[p, :, a].tobytes(), "little") for a in range(n)]
            for p in range(resid.shape[0])]
    for a in range(0, n, 7):
        c = 0
        for k in np.flatnonzero(~bits[a]):
            kind, p = int(table[k]) >> 16, int(table[k]) & 0xFFFF
            c += 1 if kind == FLAT else max(1, bin(ints[p][a]).count("1")) if kind == HAMMING \
                else 1 + ints[p][a].bit_length()
        assert c == cost[a]
    assert int(cost.max()) <= n_roots * 257 < 1 << 19
    nf, co = walk_score_host(masks, None, RP.flat_table(n_roots), n_roots)
    assert np.array_equal(nf, want_nfail) and np.array_equal(co, want_nfail)


def test_host_entry_refusals():
    lib = load_library()
    bits, resid, table = score_inputs(33, 16, 5)
    masks = pack_masks(bits)
    walk_score_host(masks, resid, table, 33)
    for bad in (np.uint32(3 << 16), np.uint32(HAMMING << 16 | resid.shape[0]),
                np.uint32(MAGNITUDE << 16 | 0xFFFF)):
        t = table.copy()
        t[7] = bad
        with pytest.raises(EngineError, match=r"\(-1\)"):
            walk_score_host(masks, resid, t, 33)
    with pytest.raises(EngineError):
        walk_score_host(masks, resid, table[:0], 0)
    with pytest.raises(EngineError):                                 # a residual kind, no residuals
        walk_score_host(masks, None, table, 33)
    big = np.zeros(1025, dtype=np.uint32)
    with pytest.raises(EngineError):
        walk_score_host(pack_masks(np.ones((4, 1025), dtype=bool)), None, big, 1025)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nf, co = np.zeros(16, dtype=np.uint32), np.zeros(16, dtype=np.uint32)
    good = [p(masks), p(resid), p(table), 33, resid.shape[0], 16, p(nf), p(co)]
    assert lib.mg_walk_score_host(*good) == 0
    for k in (0, 1, 2, 6, 7):
        q = list(good)
        q[k] = None
        assert lib.mg_walk_score_host(*q) == -1


def same_as_repair(walk, rep):
    assert walk.leaves.shape[0] == 1 and walk.winner == 0
    assert np.array_equal(walk.leaves[0], rep.leaves)
    assert int(walk.nfail[0]) == rep.nfail == int(walk.cost[0])
    assert walk.rounds == rep.rounds
    assert np.array_equal(walk.trace[0, :, 0], rep.trace)
    assert np.array_equal(walk.trace[0, :, 1], rep.trace)             # all FLAT: cost == nfail


def flat_walk_of_repair_case(name, lanes, rounds, sync_every=8):
    prog = RK.masked_program(name)
    bits = RK.bits_fn(name)
    values = lambda soa: (bits(soa), np.zeros((0, 8, soa.shape[2]), dtype=np.uint32))
    return RP.walk_ref(values, default_leafgen(prog), RK.consts_of(prog),
                       RK.start_rows(name)[None], RP.flat_table(len(RK.case(name)[0])), RK.SEED,
                       lanes, rounds, sync_every)


@pytest.mark.parametrize("name", RK.NAMES)
def test_one_flat_walker_is_the_existing_walker(name):
    same_as_repair(flat_walk_of_repair_case(name, 1000, 24), RK.reference(name, 1000, 24))
    if name in ("bytes", "narrow"):                      # to a model, at the case's own width
        rep = RK.reference(name)
        assert rep.nfail == 0 and rep.rounds < RK.MAX_ROUNDS
        same_as_repair(flat_walk_of_repair_case(name, RK.LANES, RK.MAX_ROUNDS), rep)


@pytest.mark.parametrize("name,walkers,lanes,rounds", [("magnitude", 3, 256, 16),
                                                       ("hamming", 2, 1000, 8)])
def test_walkers_are_single_walkers_with_their_own_seeds(name, walkers, lanes, rounds):
    res = K.reference(name, walkers, lanes, rounds)
    prog = K.program(name)
    assert res.leaves.shape == (walkers, len(prog.leaves), 8)
    assert len({res.leaves[w].tobytes() for w in range(walkers)}) == walkers    # they differ
    for w in range(walkers):
        one = RP.walk_ref(K.values_fn(name), default_leafgen(prog), K.consts_of(prog),
                          K.starts(name, 1), K.scoring(name)[1], K.SEED ^ (w * RP.CW & RP.M64),
                          lanes, res.rounds, res.rounds)
        assert one.rounds == res.rounds
        assert np.array_equal(one.leaves[0], res.leaves[w])
        assert (one.nfail[0], one.cost[0]) == (res.nfail[w], res.cost[w])
        assert np.array_equal(one.trace[0, :res.rounds], res.trace[w, :res.rounds])
    assert not res.trace[:, res.rounds:].any()
    keys = [(int(res.nfail[w]), int(res.cost[w]), w) for w in range(walkers)]
    assert res.winner == min(keys)[2]
    if res.rounds < rounds:                              # stopped: some walker has a model
        assert res.rounds % 8 == 0 and res.nfail.min() == 0
    assert RP.CW % 2 == 1 and RP.CW < 1 << 64


@pytest.mark.parametrize("name", K.NAMES)
def test_crafted_cases_need_the_gradient(name):
    """The conditions on the inputs, none of them a measurement: (a) the
    generator finds no model among lanes x max_rounds candidates, (b) the
    count alone (repair_ref) is still failing after max_rounds from the same
    start, (c) walk_ref reaches a model within half of max_rounds."""
    rounds = K.MAX_ROUNDS[name]
    scored, flat = K.program(name), K.program(name, 16, True)
    assert [l.source for l in scored.leaves] == [l.source for l in flat.leaves]
    assert scored.const_values == flat.const_values          # the same moves on both
    kinds = set((K.scoring(name)[1] >> 16).tolist())
    assert kinds == {"hamming": {FLAT, HAMMING}, "magnitude": {FLAT, MAGNITUDE},
                     "mixed": {FLAT, HAMMING, MAGNITUDE}}[name]
    start = K.start_rows(name)
    bits = K.bits_fn(name)
    assert int((~bits(start[:, :, None])[0]).sum()) == (9 if name == "mixed" else 1)
    assert K.generator_hits(name, K.LANES * rounds) == 0                          # (a)
    count = K.count_reference(name)
    assert count.nfail > 0 and count.rounds == rounds                             # (b)
    res = K.reference(name)
    zero = np.flatnonzero(res.trace[0, :res.rounds, 0] == 0)
    assert zero.size and int(zero[0]) < rounds // 2                               # (c)
    assert int(zero[0]) == K.FIRST_ZERO[name]                 # what the cases' docstring says
    assert res.nfail[0] == 0 == res.cost[0] and res.winner == 0 and res.rounds % 8 == 0
    assert bits(np.asarray(res.leaves[0])[:, :, None])[0].all()
    keys = res.trace[0, :res.rounds].astype(np.int64)
    keys = keys[:, 0] << 20 | keys[:, 1]
    assert (np.diff(keys) <= 0).all() and (np.diff(keys) < 0).sum() >= 2          # a descent

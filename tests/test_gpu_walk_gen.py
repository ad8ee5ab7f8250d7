"""The repair walks on the GPU past one mask word, one mask probe and one pass
of the grid (mg_repair, mg_walk, mg_walk_tree, mg_walk_aim):
Engine.repair, Engine.walk, Engine.walk_tree and Engine.walk_aim against
repair_ref and walk_ref through the oracle (oracle/evalref.c), bit for bit in
every output, on the generated cases (tests/gen_cases.py; their conditions:
tests/test_gen_cases.py) on both register layouts, every walker from a start
of its own; and one round of each kernel over 786433 lanes, 3073 tiles on 2048
blocks, whose adopted lane lies in the second trip of the strided loops.

CPU time of the references of the strided tests (cached, shared by both
layouts), measured on the host of an MI355X: repair 3.0 s, walk 4.0 s,
walk_tree 5.4 s, walk_aim (two rounds) 9.8 s."""

import numpy as np
import pytest

import gen_cases as G
from gpu_batch import oracle_inputs
from mythril_amd import census as CS
from mythril_amd import repair as RP
from mythril_amd.engine import default_leafgen, get_engine

pytestmark = pytest.mark.gpu

KERNELS = ("walk_tree", "walk", "walk_aim", "repair")
SCORING = {"walk_tree": "tree", "walk": "table", "walk_aim": "tree", "repair": "mask"}


def loaded(name, nreg, scoring):
    """(engine of the layout, the case's program of ``scoring`` loaded with
    the default generator, root count)."""
    prog, ref = G.program(name, nreg, scoring), G.program(name, 16, scoring)
    assert oracle_inputs(prog) == oracle_inputs(ref)    # the reference ran on these tables
    assert [(l.kind, l.source, l.chunk, l.width) for l in prog.leaves] == \
        [(l.kind, l.source, l.chunk, l.width) for l in ref.leaves]
    T, n_roots = G.trees(name), len(G.case(name))
    extra = {"tree": CS.n_mask_probes(T.n_atoms) + T.n_resid,
             "table": len(G.table_scoring(name)[0]), "mask": 0}[scoring]
    assert prog.n_probes == CS.n_mask_probes(n_roots) + extra
    eng = get_engine(0, nreg=nreg)
    assert eng.nreg == nreg
    return eng, eng.load(prog, default_leafgen(prog), prog_seed=0), n_roots


def same(got, want):
    assert np.array_equal(got.leaves, want.leaves)
    assert np.array_equal(got.nfail, want.nfail) and np.array_equal(got.cost, want.cost)
    assert got.winner == want.winner and got.rounds == want.rounds
    assert np.array_equal(got.trace, want.trace)


def same_repair(got, want):
    assert np.array_equal(got.leaves, want.leaves)
    assert got.nfail == want.nfail and got.rounds == want.rounds
    assert np.array_equal(got.trace, want.trace)


def run(eng, lp, kernel, name, n_roots, starts, seed, lanes, rounds):
    T = G.trees(name)
    if kernel == "repair":
        return eng.repair(lp, starts[0], n_roots, seed, lanes, rounds)
    if kernel == "walk":
        probes, table = G.table_scoring(name)
        return eng.walk(lp, starts, n_roots, table, len(probes), seed, lanes, rounds)
    if kernel == "walk_tree":
        return eng.walk_tree(lp, starts, n_roots, T, seed, lanes, rounds)
    return eng.walk_aim(lp, starts, n_roots, T, G.aims(name), seed, lanes, rounds)


@pytest.mark.parametrize("nreg", (16, 11))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", G.NAMES)
def test_the_kernels_equal_the_reference(name, kernel, nreg):
    scoring = SCORING[kernel]
    eng, lp, n_roots = loaded(name, nreg, scoring)
    assert len(G.case("ladder_ne")) == len(G.case("ladder_lt")) == 257
    assert G.trees("ladder_ne").is_tree(256) and G.trees("ladder_lt").is_tree(256)
    assert G.trees("flats").n_atoms > 256
    if kernel == "walk_aim":
        assert name != "rules" or len(G.aims(name)) > 0
    timed = False
    for lanes, walkers in G.SHAPES:
        # the census-view limit of the C ABI: the (256, 64) shape of ladder_lt is 130 MiB
        assert lanes * walkers * lp.program.n_probes * 32 < 256 << 20
        rounds = G.rounds_at(name, (lanes, walkers))
        starts = G.starts(name, walkers, scoring)
        got = run(eng, lp, kernel, name, n_roots, starts, G.SEED, lanes, rounds)
        if kernel == "repair":
            assert got.trace.shape == (rounds,)
            same_repair(got, G.repair_reference(name, lanes, rounds))
        else:
            which = {"walk": "table", "walk_tree": "tree", "walk_aim": "aim"}[kernel]
            want = G.reference(name, walkers, lanes, rounds, which)
            assert got.trace.shape == (walkers, rounds, 2)
            assert got.leaves.shape == want.leaves.shape
            same(got, want)
            if kernel == "walk_aim" and not len(G.aims(name)):     # no entry: mg_walk_tree
                same(got, eng.walk_tree(lp, starts, n_roots, G.trees(name), G.SEED, lanes, rounds))
        timed = timed or got.kernel_ms > 0
    assert timed


# ---------------------------------------------------------------------------
# the second trip of the strided loops
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("nreg", (16, 11))
@pytest.mark.parametrize("kernel", ("repair", "walk", "walk_tree", "walk_aim"))
def test_the_adopted_lane_of_a_second_tile(kernel, nreg):
    """786433 lanes of one walker: blocks 0 .. 1024 of mutate and of score or
    select take a second tile, the last tile has one active lane, and the lane
    the round adopts is in the second trip, alone at its key: the key
    reduction, the adopt step's recomputation from the lane number and (for
    mg_walk_aim) its gather of the lane's residual column all see it."""
    seed, rnd, lane = G.STRIDE_SEEDS[kernel]
    lanes = G.STRIDE_LANES
    assert lanes == 3 * (1 << 18) + 1 and (lanes + 255) // 256 == 3073 > 2048
    want, best, at_key, key = G.stride_reference(kernel)
    assert best == lane >= 2048 * 256 and at_key == 1
    trace = np.asarray(want.trace).reshape(-1, 2 if kernel != "repair" else 1)
    assert tuple(trace[rnd]) == (key if kernel != "repair" else key[:1])      # .. and adopted:
    assert rnd == 0 or tuple(trace[rnd]) < tuple(trace[rnd - 1])              # strictly better
    if kernel == "walk_aim":
        assert rnd == 1 and len(G.aims(G.STRIDE)) > 0
        # round 0 finds nothing better than the start (lane 0), so round 1 leaves from
        # it, and under its residual values the round has aimed lanes
        vals = G.values_fn(G.STRIDE)(np.ascontiguousarray(G.starts(G.STRIDE, 1)[0][:, :, None]))
        nf, co = RP.tree_scoring(G.trees(G.STRIDE))(*vals)
        assert tuple(trace[0]) == (int(nf[0]), int(co[0])) and nf[0] > 0
        picks = RP.aim_picks_ref(vals[2][:, :, 0], G.aims(G.STRIDE), 1, lanes)
        assert (picks != RP.AIM_NONE).sum() >= 2
    eng, lp, n_roots = loaded(G.STRIDE, nreg, SCORING[kernel])
    assert lanes * lp.program.n_probes * 32 < 256 << 20
    starts = G.starts(G.STRIDE, 1, SCORING[kernel])
    got = run(eng, lp, kernel, G.STRIDE, n_roots, starts, seed, lanes, rnd + 1)
    (same_repair if kernel == "repair" else same)(got, want)
    assert not np.array_equal(np.asarray(got.leaves).reshape(starts.shape), starts)
    assert got.kernel_ms > 0

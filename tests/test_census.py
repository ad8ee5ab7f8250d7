"""The verdict census on the CPU (mythril_amd/census.py): the
mask probes through the IR simulator against the oracle's per-constraint
bits, reduce_masks (the kernel's specification) against a lane-by-lane
recount, the census view, and the library export."""

import numpy as np
import pytest

import census_cases as K
import ir_sim
from mythril_amd import census as CS
from mythril_amd import irdefs as I
from mythril_amd.ir import compile_constraints
from mythril_amd.smt import node as N
from oracle import gen_ref

SIM_LANES = 192          # three class groups of the generator
CASES = [("ladder", R) for R in K.RS] + [("c2", 7), ("c4", 16)]


def sim_lane(prog, idx, seed=K.SEED, prog_seed=K.PROG_SEED):
    leaves = [gen_ref.gen_leaf(seed, prog_seed, li, idx, l.width, prog.const_values)
              for li, l in enumerate(prog.leaves)]
    return ir_sim.run(prog, leaves)


def assert_fixture_is_telling(key, bits):
    """Asserted from the oracle alone, before anything is compared with it:
    the range has satisfying lanes, sole-blocker lanes and first blockers
    spread over the roots (else the census fields compared are trivial)."""
    R = bits.shape[1]
    nfail = (~bits).sum(axis=1)
    assert (nfail == 0).sum() >= 1, key
    assert (nfail == 1).sum() >= 1, key
    assert len(set(np.argmax(~bits, axis=1)[nfail > 0])) >= R / 2, key


@pytest.mark.parametrize("key", CASES, ids=lambda k: "%s%d" % k)
def test_mask_probes_equal_the_oracle_per_root(key):
    cs, prog = K.masked_program(key)
    n_mask = CS.n_mask_probes(len(cs))
    assert prog.n_user_probes == prog.n_probes == n_mask
    assert n_mask == (2 if len(cs) > 256 else 1)
    bits = K.oracle_bits(key, K.FIRST, SIM_LANES)
    for i in range(SIM_LANES):
        root, probes = sim_lane(prog, K.FIRST + i)
        value = sum(p << (256 * j) for j, p in enumerate(probes))
        want = sum(int(b) << k for k, b in enumerate(bits[i]))
        assert value == want, (key, i)
        assert root == int(bits[i].all()), (key, i)


@pytest.mark.parametrize("R", K.RS)
def test_reduce_masks_equals_a_recount_of_the_oracle(R):
    key = ("ladder", R)
    bits = K.oracle_bits(key)
    assert bits.shape == (K.N_CAND, R)
    assert_fixture_is_telling(key, bits)
    c = CS.reduce_masks(K.pack_masks(bits), R, K.FIRST)
    assert c.as_dict() == K.recount(bits, K.FIRST)
    assert c.n_sat == int(bits.all(axis=1).sum()) > 0
    assert c.first_sat == K.FIRST + int(np.argmax(bits.all(axis=1))) and c.best_nfail == 0
    # the identities
    assert int(c.first_block.sum()) + c.n_sat == c.n_cand == K.N_CAND
    assert int(c.sole_block.sum()) == int(c.nfail_hist[1])
    assert (c.sole_block <= c.first_block).all()
    assert (c.first_block <= c.n_cand - c.pass_).all()
    assert int(c.nfail_hist.sum()) == c.n_cand
    c.check()


def test_reduce_masks_ignores_bits_at_or_above_n_roots():
    bits = K.oracle_bits(("ladder", 33))
    assert bits[:, 20:].any()                  # set bits above the 20 roots counted
    c = CS.reduce_masks(K.pack_masks(bits), 20, K.FIRST)
    assert c.as_dict() == K.recount(bits[:, :20], K.FIRST)
    ones = np.full((2, 8, 5), 0xFFFFFFFF, dtype=np.uint32)
    c = CS.reduce_masks(ones, 257, 0)
    assert c.n_sat == 5 and int(c.first_block.sum()) == 0 and c.nfail_hist.shape == (258,)


def test_empty_range_and_merge_and_blockers():
    bits = K.oracle_bits(("ladder", 65))
    whole = CS.reduce_bits(bits, K.FIRST)
    a, b = CS.reduce_bits(bits[:448], K.FIRST), CS.reduce_bits(bits[448:], K.FIRST + 448)
    assert a.merge(b) == whole == b.merge(a)
    empty = CS.reduce_bits(bits[:0], K.FIRST)
    assert (empty.best_nfail, empty.best_index, empty.n_sat, empty.first_sat) == (66, -1, 0, -1)
    assert (empty.sole_index == -1).all() and empty.merge(whole) == whole
    # never-satisfied roots first, then by sole_block, then by first_block
    # (root 0 always holds: no blocker; root 3 never does)
    c = CS.reduce_bits(np.array([[1, 0, 1, 0], [1, 0, 0, 0], [1, 1, 1, 0], [1, 1, 1, 0],
                                 [1, 0, 0, 0]], dtype=bool), 0)
    assert c.blockers() == [3, 1, 2]
    assert list(c.sole_block) == [0, 0, 0, 2] and list(c.first_block) == [0, 3, 0, 2]
    c = CS.reduce_bits(np.array([[0, 1, 1], [1, 0, 1], [1, 0, 1], [1, 1, 0], [0, 0, 1],
                                 [1, 1, 1]], dtype=bool), 64)
    assert list(c.sole_block) == [1, 2, 1] and list(c.first_block) == [2, 2, 1]
    assert c.blockers() == [1, 0, 2]
    assert list(c.sole_index) == [64, 65, 67] and (c.first_sat, c.n_sat) == (69, 1)


def test_census_view_keeps_the_root_and_the_mask():
    cs = K.ladder(33)
    x, z = N.bv_var("x", 16), N.bv_var("z", 16)
    mask = CS.mask_probes(cs)
    prog = compile_constraints(cs, mask + [N.bv_op("bvadd", x, z), z])
    assert prog.n_probes == 3
    view = CS.census_view(prog, 1)
    assert view.n_probes == 1 and prog.n_probes == 3         # the program is untouched
    outs = view.code[(view.code[:, 0] & 0xFF) == I.OUT]
    assert len(outs) == 1 and int(outs[0, 2]) == 0
    assert ((view.code[:, 0] & 0xFF) == I.NOP).sum() == ((prog.code[:, 0] & 0xFF) == I.NOP).sum() + 2
    assert view.const_values == prog.const_values and len(view.leaves) == len(prog.leaves)
    for i in range(64):
        root, probes = sim_lane(prog, K.FIRST + i)
        vroot, vprobes = sim_lane(view, K.FIRST + i)
        assert (vroot, vprobes) == (root, probes[:1])
    with pytest.raises(ValueError):
        CS.census_view(prog, 4)


def test_census_view_of_a_search_program_in_the_assembly_simulator():
    """A search-form program (C4 query 16: 130 probes, one of them the mask)
    and its view through the assembly interpreter's simulator, one wave of
    the search generator: same root bits, same mask, and the root bit is the
    AND of the mask's bits (under the constructed model)."""
    import asm_sim
    import mythril_amd.model as M
    from mythril_amd import workloads as W
    group = max(M.dependence_buckets(W.queries("c4", 64)[16]), key=len)
    full = M._compile_search_uncached(group, CS.mask_probes(group))
    assert full.n_user_probes == 1 and full.n_probes > 100 and full.solved
    view = CS.census_view(full, 1)
    gen = (M.SEARCH_SEED, 0, 128, M.search_leafgen(full))
    root, probes, _, _ = asm_sim.simulate(full, gen=gen)
    vroot, vprobes, _, _ = asm_sim.simulate(view, gen=gen)
    assert vprobes.shape == (1, 8, 64)
    assert (vroot == root).all() and (vprobes == probes[:1]).all()
    assert (CS.mask_bits(vprobes, len(group)).all(axis=1) == vroot).all()


def test_library_exports_mg_census():
    from mythril_amd import engine
    assert "mg_census" in engine.EXPORTS
    lib = engine.load_library()
    assert lib.mg_census.argtypes is not None and len(lib.mg_census.argtypes) == 14

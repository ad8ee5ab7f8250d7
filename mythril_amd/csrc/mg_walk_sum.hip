// mg_walk_bound, mg_walk_uf, mg_walk_sum — the tree-scored walks with moves
// aimed by a failing equality's residual or a failing order's difference
// (DESIGN.md §3.13), through the table entry a UF application reads (§3.14) and
// through sums, differences, masks and shifts (§3.15); specification:
// mythril_amd/repair.py walk_ref with bounds, ufs and sums.
//
// The three rungs are nested (mg_walk_sum.h), so one round serves them all: a
// lower rung runs it with lin words all 0, no side row, no slot and no U row.
// A round is the round of mg_walk_aim.hip with its two kernels exchanged:
//   mg_walk_sum_mutate  lane j of walker w writes neighbour j of base w: the
//                       lane function of mg_walk_sum.h, which reads the
//                       walker's residual values, side rows sstate[w][n_srows]
//                       [8], live list and slot destinations dest[w][n_slots]
//                       (all wave-uniform per walker) and the lin words of the
//                       entries
//   the interpreter     writes every neighbour's root mask, atom mask,
//                       residual probes, side rows and U rows (the arguments'
//                       chunks, then the computed keys of argument-keyed
//                       entries)
//   mg_walk_tree_score  (mg_walk_tree.hip, unchanged)
//   mg_walk_sum_adopt   block w: what mg_walk_aim_adopt does for walker w; on
//                       adoption the block also gathers the adopted lane's
//                       root-mask and atom-mask rows (at most (4 + 4) x 8
//                       words), side rows and U rows into the walker's state
//                       next to the residual rows, resolves every slot, one
//                       thread per slot, against the updated base and that
//                       lane's U rows (after the barrier that makes thread 0's
//                       in-place update of the base visible), and rebuilds the
//                       live list under the rule of mg_walk_uf.h, one thread
//                       per entry ranked by prefix count: L stays in table
//                       order whatever the schedule
// The bodies of the kernels live in mg_walk_round.h: mg_walk_batch.hip runs
// them too.  Thread 0 applies the adopted lane under the OLD side rows, before
// the barrier; the block replaces them after it, as it replaces the residual
// values.  The walkers' states start at ~0, so round 0 always adopts and the
// residuals, masks, side rows and U rows are known from round 1 on; the
// destinations start at MG_AIM_NONE and the live lists empty, so before round
// 0's adoption no entry is live and nothing of them is read.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_walk_round.h"

__global__ __launch_bounds__(MG_WALK_BLOCK) void mg_walk_sum_mutate(
    const uint32_t* __restrict__ bases, const mg_leafgen* __restrict__ gen,
    const uint32_t* __restrict__ consts, uint32_t n_leaves, uint64_t seed, uint32_t r,
    uint32_t lanes, const uint32_t* __restrict__ entries, const uint32_t* __restrict__ pieces,
    const uint32_t* __restrict__ fixed, const uint32_t* __restrict__ lin,
    const uint32_t* __restrict__ rstate, uint32_t n_resid, const uint32_t* __restrict__ sstate,
    uint32_t n_srows, const uint32_t* __restrict__ lives, const uint32_t* __restrict__ dests,
    uint32_t n_slots, uint32_t* out) {
    mg_walk_mutate_body(bases, gen, consts, n_leaves, seed, r, lanes, entries, pieces, fixed, lin,
                        rstate, n_resid, sstate, n_srows, lives, dests, n_slots, out);
}

__global__ __launch_bounds__(MG_WALK_BLOCK) void mg_walk_sum_adopt(
    uint32_t* bases, const mg_leafgen* __restrict__ gen, const uint32_t* __restrict__ consts,
    uint32_t n_leaves, uint64_t seed, uint32_t r, uint32_t lanes, uint32_t max_rounds,
    const uint32_t* __restrict__ entries, uint32_t n_entries,
    const uint32_t* __restrict__ pieces, const uint32_t* __restrict__ fixed,
    const uint32_t* __restrict__ lin, const uint32_t* __restrict__ resid, uint32_t n_resid,
    const uint32_t* __restrict__ masks, uint32_t n_mwords, uint32_t n_rwords,
    const uint32_t* __restrict__ srows, uint32_t n_srows, uint32_t* sstate,
    const uint32_t* __restrict__ urows, uint32_t n_urows,
    const uint32_t* __restrict__ slots, uint32_t n_slots, const uint32_t* __restrict__ funcs,
    const uint32_t* __restrict__ cands, const uint32_t* __restrict__ ukeys, uint32_t* rstate,
    uint32_t* mstate, uint32_t* ustate, uint32_t* dests, uint32_t* lives,
    mg_walk_state* __restrict__ st, uint32_t* __restrict__ trace) {
    mg_walk_adopt_body(blockIdx.y, (size_t)gridDim.y * lanes, bases, gen, consts, n_leaves, seed, r,
                       lanes, max_rounds, entries, n_entries, pieces, fixed, lin, resid, n_resid,
                       masks, n_mwords, n_rwords, srows, n_srows, sstate, urows, n_urows, slots,
                       n_slots, funcs, cands, ukeys, rstate, mstate, ustate, dests, lives, st,
                       trace);
}

static bool sum_shape_ok(uint32_t walkers, uint32_t lanes, uint32_t n_leaves, uint32_t r,
                         uint32_t n_entries, uint32_t n_slots, uint32_t n_urows,
                         uint32_t n_srows) {
    return walkers >= 1 && walkers <= MG_WALK_MAX_WALKERS && lanes >= 1 &&
           lanes <= MG_REPAIR_MAX_LANES && n_leaves > 0 && r < MG_REPAIR_MAX_ROUNDS &&
           n_entries <= MG_AIM_MAX_ENTRIES && n_slots <= MG_UF_MAX_SLOTS &&
           n_urows <= MG_UF_MAX_ROWS && n_srows <= MG_SUM_MAX_ROWS;
}

// The tables must have passed mg_walk_sum_ok (every rung's entry checks them
// before it uploads); d_rstate, d_lives as mg_launch_walk_aim_round, d_dests:
// [walkers][n_slots], MG_AIM_NONE before round 0, d_sstate: [walkers][n_srows]
// [8], d_lin: [n_entries], zero for a lower rung.
hipError_t mg_launch_walk_sum_round(const uint32_t* d_bases, const mg_leafgen* d_gen,
                                   const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                                   uint32_t r, uint32_t lanes, uint32_t walkers,
                                   const uint32_t* d_entries, uint32_t n_entries,
                                   const uint32_t* d_pieces, const uint32_t* d_fixed,
                                   const uint32_t* d_lin, const uint32_t* d_rstate,
                                   uint32_t n_resid, const uint32_t* d_sstate, uint32_t n_srows,
                                   const uint32_t* d_lives, const uint32_t* d_dests,
                                   uint32_t n_slots, uint32_t* d_leaves, hipStream_t stream) {
    if (!sum_shape_ok(walkers, lanes, n_leaves, r, n_entries, n_slots, 0, n_srows))
        return hipErrorInvalidValue;
    const uint32_t blocks = mg_walk_grid_blocks(lanes);
    hipLaunchKernelGGL(mg_walk_sum_mutate, dim3(blocks, walkers), dim3(MG_WALK_BLOCK), 0, stream,
                       d_bases, d_gen, d_consts, n_leaves, seed, r, lanes, d_entries, d_pieces,
                       d_fixed, d_lin, d_rstate, n_resid, d_sstate, n_srows, d_lives, d_dests,
                       n_slots, d_leaves);
    return hipGetLastError();
}

// score with the tree tables (the kernel of mg_walk_tree.hip), then the adopt
// of this file.  d_amasks follows d_masks, d_srows the n_resid residual rows
// of d_resid and d_urows the n_srows side rows in the probe buffer.  uf: the
// device copies of the UF tables.
hipError_t mg_launch_walk_sum_pick(const uint32_t* d_masks, const uint32_t* d_amasks,
                                  const uint32_t* d_resid, const uint32_t* d_srows,
                                  uint32_t n_srows, const uint32_t* d_urows,
                                  const uint32_t* d_roots, const uint32_t* d_atoms,
                                  const uint32_t* d_code, uint32_t lanes, uint32_t walkers,
                                  uint32_t n_roots, uint32_t n_atoms, uint32_t* d_bases,
                                  const mg_leafgen* d_gen, const uint32_t* d_consts,
                                  uint32_t n_leaves, uint64_t seed, uint32_t r,
                                  uint32_t max_rounds, const uint32_t* d_entries,
                                  uint32_t n_entries, const uint32_t* d_pieces,
                                  const uint32_t* d_fixed, const uint32_t* d_lin,
                                  uint32_t n_resid, const mg_uf_tables& uf, uint32_t* d_rstate,
                                  uint32_t* d_mstate, uint32_t* d_sstate, uint32_t* d_ustate,
                                  uint32_t* d_dests, uint32_t* d_lives, mg_walk_state* d_state,
                                  uint32_t* d_trace, hipStream_t stream) {
    const uint32_t n_rwords = MG_BOUND_MASK_WORDS(n_roots),
                   n_mwords = n_rwords + MG_BOUND_MASK_WORDS(n_atoms);
    if (!sum_shape_ok(walkers, lanes, n_leaves, r, n_entries, uf.n_slots, uf.n_urows, n_srows) ||
        n_roots == 0 || n_roots > MG_WT_MAX_ROOTS || n_atoms > MG_WT_MAX_ATOMS ||
        r >= max_rounds || d_amasks != d_masks + (size_t)n_rwords * walkers * lanes ||
        d_srows != d_resid + (size_t)n_resid * 8 * walkers * lanes ||
        d_urows != d_srows + (size_t)n_srows * 8 * walkers * lanes)
        return hipErrorInvalidValue;
    const uint32_t blocks = mg_walk_grid_blocks(lanes);
    hipLaunchKernelGGL(mg_walk_tree_score, dim3(blocks, walkers), dim3(MG_WALK_BLOCK), 0, stream,
                       d_masks, d_amasks, d_resid, d_roots, d_atoms, d_code, lanes, n_roots,
                       d_state);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mg_walk_sum_adopt, dim3(1, walkers), dim3(MG_WALK_BLOCK), 0, stream,
                       d_bases, d_gen, d_consts, n_leaves, seed, r, lanes, max_rounds, d_entries,
                       n_entries, d_pieces, d_fixed, d_lin, d_resid, n_resid, d_masks, n_mwords,
                       n_rwords, d_srows, n_srows, d_sstate, d_urows, uf.n_urows, uf.slots,
                       uf.n_slots, uf.funcs, uf.cands, uf.ukeys, d_rstate, d_mstate, d_ustate,
                       d_dests, d_lives, d_state, d_trace);
    return hipGetLastError();
}

// mg_walk_sum — the tree-scored walk with aims through sums, differences,
// masks and shifts (specification: mythril_amd/repair.py
// walk_ref with sums).
//
// A round is the round of mg_walk_uf.hip with its two kernels exchanged:
//   mg_walk_sum_mutate  mg_walk_sum_mutate with the lin words of the entries
//                       and one more wave-uniform input per walker: the side
//                       rows sstate[w][n_srows][8] of its base (the lane
//                       function of mg_walk_sum.h)
//   the interpreter     writes every neighbour's root mask, atom mask,
//                       residual probes, side rows and U rows
//   mg_walk_tree_score  (mg_walk_tree.hip, unchanged)
//   mg_walk_sum_adopt   mg_walk_sum_adopt; on adoption the block also gathers
//                       the adopted lane's side rows into the walker's state
// (the adopt body lives in mg_walk_batch.h: mg_walk_batch_adopt runs it too).
// Thread 0 applies the adopted lane under the OLD side rows, before the
// barrier; the block replaces them after it, as it replaces the residual
// values.  Before round 0's adoption no entry is live and nothing is read.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_walk_batch.h"      // the adopt body, shared with mg_walk_batch_adopt
#include "mg_walk_sum.h"
#include "mg_walk_tree.h"

#define BLOCK MG_WALK_BLOCK
// blocks per walker and launch: tiles beyond are grid-strided (as mg_walk.hip)
#define MAX_BLOCKS 2048u

// the score kernel of mg_walk_tree.hip
__global__ __launch_bounds__(BLOCK) void mg_walk_tree_score(
    const uint32_t* __restrict__ masks, const uint32_t* __restrict__ amasks,
    const uint32_t* __restrict__ resid, const uint32_t* __restrict__ roots,
    const uint32_t* __restrict__ atoms, const uint32_t* __restrict__ code, uint32_t lanes,
    uint32_t n_roots, mg_walk_state* __restrict__ st);

__global__ __launch_bounds__(BLOCK) void mg_walk_sum_mutate(
    const uint32_t* __restrict__ bases, const mg_leafgen* __restrict__ gen,
    const uint32_t* __restrict__ consts, uint32_t n_leaves, uint64_t seed, uint32_t r,
    uint32_t lanes, const uint32_t* __restrict__ entries, const uint32_t* __restrict__ pieces,
    const uint32_t* __restrict__ fixed, const uint32_t* __restrict__ lin,
    const uint32_t* __restrict__ rstate, uint32_t n_resid, const uint32_t* __restrict__ sstate,
    uint32_t n_srows, const uint32_t* __restrict__ lives, const uint32_t* __restrict__ dests,
    uint32_t n_slots, uint32_t* out) {
    const uint32_t w = blockIdx.y;
    const size_t total = (size_t)gridDim.y * lanes;
    const uint32_t* base = bases + (size_t)w * n_leaves * 8;
    const uint32_t* rvals = rstate + (size_t)w * n_resid * 8;
    const uint32_t* svals = sstate + (size_t)w * n_srows * 8;
    const uint32_t* live = lives + (size_t)w * MG_AIM_LIVE_WORDS;
    const uint32_t* dest = dests + (size_t)w * n_slots;
    const uint64_t wseed = mg_walk_seed(seed, w);
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // uniform per block
        const uint32_t j = tile * BLOCK + threadIdx.x;
        if (j >= lanes) continue;
        uint32_t* col = out + (size_t)w * lanes + j;
        for (uint32_t leaf = 0; leaf < n_leaves; ++leaf)
            for (uint32_t k = 0; k < 8; ++k)                               // one row: coalesced
                col[((size_t)leaf * 8 + k) * total] = base[(size_t)leaf * 8 + k];
        // the lane's own column again: its pieces applied, its moves over them
        mg_walk_sum_lane(base, gen, consts, n_leaves, wseed, r, j, lanes, entries, pieces, fixed,
                         lin, rvals, svals, live, dest, col, total, nullptr);
    }
}

// masks: as mg_walk_bound_adopt; srows: the n_srows probes after the
// residuals, urows: the n_urows probes after them; sstate: [walkers][n_srows][8],
// ustate: [walkers][n_urows][8], dests: [walkers][n_slots]
__global__ __launch_bounds__(BLOCK) void mg_walk_sum_adopt(
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
    mg_walk_sum_adopt_body(blockIdx.y, (size_t)gridDim.y * lanes, bases, gen, consts, n_leaves,
                           seed, r, lanes, max_rounds, entries, n_entries, pieces, fixed, lin,
                           resid, n_resid, masks, n_mwords, n_rwords, srows, n_srows, sstate,
                           urows, n_urows, slots, n_slots, funcs, cands, ukeys, rstate, mstate,
                           ustate, dests, lives, st, trace);
}

static bool sum_shape_ok(uint32_t walkers, uint32_t lanes, uint32_t n_leaves, uint32_t r,
                         uint32_t n_entries, uint32_t n_slots, uint32_t n_urows,
                         uint32_t n_srows) {
    return walkers >= 1 && walkers <= MG_WALK_MAX_WALKERS && lanes >= 1 &&
           lanes <= MG_REPAIR_MAX_LANES && n_leaves > 0 && r < MG_REPAIR_MAX_ROUNDS &&
           n_entries <= MG_AIM_MAX_ENTRIES && n_slots <= MG_UF_MAX_SLOTS &&
           n_urows <= MG_UF_MAX_ROWS && n_srows <= MG_SUM_MAX_ROWS;
}

// The tables must have passed mg_walk_sum_ok (mg_walk_sum checks them before
// it uploads); d_rstate, d_lives as mg_launch_walk_bound_round, d_dests as
// mg_launch_walk_uf_round, d_sstate: [walkers][n_srows][8].
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
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    const uint32_t blocks = tiles < MAX_BLOCKS ? tiles : MAX_BLOCKS;
    hipLaunchKernelGGL(mg_walk_sum_mutate, dim3(blocks, walkers), dim3(BLOCK), 0, stream, d_bases,
                       d_gen, d_consts, n_leaves, seed, r, lanes, d_entries, d_pieces, d_fixed,
                       d_lin, d_rstate, n_resid, d_sstate, n_srows, d_lives, d_dests, n_slots,
                       d_leaves);
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
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    const uint32_t blocks = tiles < MAX_BLOCKS ? tiles : MAX_BLOCKS;
    hipLaunchKernelGGL(mg_walk_tree_score, dim3(blocks, walkers), dim3(BLOCK), 0, stream, d_masks,
                       d_amasks, d_resid, d_roots, d_atoms, d_code, lanes, n_roots, d_state);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mg_walk_sum_adopt, dim3(1, walkers), dim3(BLOCK), 0, stream, d_bases, d_gen,
                       d_consts, n_leaves, seed, r, lanes, max_rounds, d_entries, n_entries,
                       d_pieces, d_fixed, d_lin, d_resid, n_resid, d_masks, n_mwords, n_rwords,
                       d_srows, n_srows, d_sstate, d_urows, uf.n_urows, uf.slots, uf.n_slots, uf.funcs, uf.cands, uf.ukeys, d_rstate,
                       d_mstate, d_ustate, d_dests, d_lives, d_state, d_trace);
    return hipGetLastError();
}

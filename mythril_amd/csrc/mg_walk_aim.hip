// mg_walk_aim — the tree-scored walk with moves aimed by a failing equality's
// residual (specification: mythril_amd/repair.py walk_ref
// with aims).
//
// A round is the round of mg_walk_tree.hip with two kernels exchanged:
//   mg_walk_aim_mutate  lane j of walker w writes neighbour j of base w: the
//                       lane function of mg_walk_aim.h, which reads the
//                       walker's residual values and live list (both
//                       wave-uniform per walker) besides what mg_walk_mutate
//                       reads
//   the interpreter     writes every neighbour's root mask, atom mask and
//                       residual probes
//   mg_walk_tree_score  (mg_walk_tree.hip, unchanged)
//   mg_walk_aim_adopt   block w: what mg_walk_adopt does for walker w, the
//                       neighbour recomputed from its lane number with the
//                       same lane function; on adoption the block also
//                       gathers the adopted lane's residual rows ([n_resid][8],
//                       one column of the probe buffer) into the walker's
//                       state and rebuilds its live list, in table order
// The walkers' states start at ~0, so round 0 always adopts and the residuals
// are known from round 1 on; the live lists start empty.  Sums and minima
// only: the result does not depend on the order of blocks.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_walk_round.h"    // the block size, the grid and mg_walk_tree_score

#define BLOCK MG_WALK_BLOCK

__global__ __launch_bounds__(BLOCK) void mg_walk_aim_mutate(
    const uint32_t* __restrict__ bases, const mg_leafgen* __restrict__ gen,
    const uint32_t* __restrict__ consts, uint32_t n_leaves, uint64_t seed, uint32_t r,
    uint32_t lanes, const uint32_t* __restrict__ entries, const uint32_t* __restrict__ pieces,
    const uint32_t* __restrict__ rstate, uint32_t n_resid, const uint32_t* __restrict__ lives,
    uint32_t* out) {
    const uint32_t w = blockIdx.y;
    const size_t total = (size_t)gridDim.y * lanes;
    const uint32_t* base = bases + (size_t)w * n_leaves * 8;
    const uint32_t* rvals = rstate + (size_t)w * n_resid * 8;
    const uint32_t* live = lives + (size_t)w * MG_AIM_LIVE_WORDS;
    const uint64_t wseed = mg_walk_seed(seed, w);
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // uniform per block
        const uint32_t j = tile * BLOCK + threadIdx.x;
        if (j >= lanes) continue;
        uint32_t* col = out + (size_t)w * lanes + j;
        for (uint32_t leaf = 0; leaf < n_leaves; ++leaf)
            for (uint32_t k = 0; k < 8; ++k)                               // one row: coalesced
                col[((size_t)leaf * 8 + k) * total] = base[(size_t)leaf * 8 + k];
        // the lane's own column again: its pieces xored in, its moves over them
        mg_walk_aim_lane(base, gen, consts, n_leaves, wseed, r, j, lanes, entries, pieces, rvals,
                         live, col, total, nullptr);
    }
}

__global__ __launch_bounds__(BLOCK) void mg_walk_aim_adopt(
    uint32_t* bases, const mg_leafgen* __restrict__ gen, const uint32_t* __restrict__ consts,
    uint32_t n_leaves, uint64_t seed, uint32_t r, uint32_t lanes, uint32_t max_rounds,
    const uint32_t* __restrict__ entries, uint32_t n_entries,
    const uint32_t* __restrict__ pieces, const uint32_t* __restrict__ resid, uint32_t n_resid,
    uint32_t* rstate, uint32_t* lives, mg_walk_state* __restrict__ st,
    uint32_t* __restrict__ trace) {
    __shared__ uint32_t s_lane;                  // the adopted lane, or MG_AIM_NONE
    __shared__ uint32_t s_flag[BLOCK];
    const uint32_t w = blockIdx.y;
    const size_t total = (size_t)gridDim.y * lanes;
    uint32_t* rvals = rstate + (size_t)w * n_resid * 8;
    uint32_t* live = lives + (size_t)w * MG_AIM_LIVE_WORDS;
    if (threadIdx.x == 0) {
        uint32_t* base = bases + (size_t)w * n_leaves * 8;
        const unsigned long long key = st[w].key;
        const uint32_t nfail = (uint32_t)(key >> MG_WALK_NFAIL_SHIFT);
        const uint32_t cost = (uint32_t)(key >> MG_WALK_COST_SHIFT) & MG_WALK_FIELD;
        const uint32_t j = (uint32_t)key & MG_WALK_FIELD;
        const bool better = nfail < st[w].nfail || (nfail == st[w].nfail && cost < st[w].cost);
        const bool adopt = key != ~0ull && better && j < lanes;
        if (adopt) {
            // the moves are computed from the base before anything is stored;
            // the old residual values and live list are read here, before the
            // barrier, and replaced after it
            mg_walk_aim_lane(base, gen, consts, n_leaves, mg_walk_seed(seed, w), r, j, lanes,
                             entries, pieces, rvals, live, base, 1, nullptr);
            st[w].nfail = nfail;
            st[w].cost = cost;
        }
        trace[((size_t)w * max_rounds + r) * 2] = nfail;
        trace[((size_t)w * max_rounds + r) * 2 + 1] = cost;
        st[w].key = ~0ull;
        s_lane = adopt ? j : MG_AIM_NONE;
    }
    __syncthreads();
    const uint32_t j = s_lane;                                             // block-uniform
    if (j == MG_AIM_NONE) return;
    const uint32_t* column = resid + (size_t)w * lanes + j;
    for (uint32_t i = threadIdx.x; i < n_resid * 8; i += BLOCK) rvals[i] = column[(size_t)i * total];
    const uint32_t e = threadIdx.x;
    s_flag[e] = e < n_entries && mg_walk_aim_is_live(entries, e, column, total) ? 1u : 0u;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t i = 0; i < BLOCK; ++i) before += i < e ? s_flag[i] : 0u;
    if (s_flag[e]) live[1 + before] = e;
    if (e == BLOCK - 1) live[0] = before + s_flag[e];
}

static bool aim_shape_ok(uint32_t walkers, uint32_t lanes, uint32_t n_leaves, uint32_t r,
                         uint32_t n_entries) {
    return walkers >= 1 && walkers <= MG_WALK_MAX_WALKERS && lanes >= 1 &&
           lanes <= MG_REPAIR_MAX_LANES && n_leaves > 0 && r < MG_REPAIR_MAX_ROUNDS &&
           n_entries <= MG_AIM_MAX_ENTRIES;
}

// The tables must have passed mg_walk_aim_ok (mg_walk_aim checks them before
// it uploads); d_rstate: [walkers][n_resid][8], d_lives: [walkers]
// [MG_AIM_LIVE_WORDS], zero before round 0.
hipError_t mg_launch_walk_aim_round(const uint32_t* d_bases, const mg_leafgen* d_gen,
                                    const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                                    uint32_t r, uint32_t lanes, uint32_t walkers,
                                    const uint32_t* d_entries, uint32_t n_entries,
                                    const uint32_t* d_pieces, const uint32_t* d_rstate,
                                    uint32_t n_resid, const uint32_t* d_lives, uint32_t* d_leaves,
                                    hipStream_t stream) {
    if (!aim_shape_ok(walkers, lanes, n_leaves, r, n_entries)) return hipErrorInvalidValue;
    const uint32_t blocks = mg_walk_grid_blocks(lanes);
    hipLaunchKernelGGL(mg_walk_aim_mutate, dim3(blocks, walkers), dim3(BLOCK), 0, stream, d_bases,
                       d_gen, d_consts, n_leaves, seed, r, lanes, d_entries, d_pieces, d_rstate,
                       n_resid, d_lives, d_leaves);
    return hipGetLastError();
}

// score with the tree tables (the kernel of mg_walk_tree.hip; the tables must
// have passed mg_walk_tree_ok), then the adopt of this file
hipError_t mg_launch_walk_aim_pick(const uint32_t* d_masks, const uint32_t* d_amasks,
                                   const uint32_t* d_resid, const uint32_t* d_roots,
                                   const uint32_t* d_atoms, const uint32_t* d_code, uint32_t lanes,
                                   uint32_t walkers, uint32_t n_roots, uint32_t* d_bases,
                                   const mg_leafgen* d_gen, const uint32_t* d_consts,
                                   uint32_t n_leaves, uint64_t seed, uint32_t r,
                                   uint32_t max_rounds, const uint32_t* d_entries,
                                   uint32_t n_entries, const uint32_t* d_pieces, uint32_t n_resid,
                                   uint32_t* d_rstate, uint32_t* d_lives, mg_walk_state* d_state,
                                   uint32_t* d_trace, hipStream_t stream) {
    if (!aim_shape_ok(walkers, lanes, n_leaves, r, n_entries) || n_roots == 0 ||
        n_roots > MG_WT_MAX_ROOTS || r >= max_rounds)
        return hipErrorInvalidValue;
    const uint32_t blocks = mg_walk_grid_blocks(lanes);
    hipLaunchKernelGGL(mg_walk_tree_score, dim3(blocks, walkers), dim3(BLOCK), 0, stream, d_masks,
                       d_amasks, d_resid, d_roots, d_atoms, d_code, lanes, n_roots, d_state);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mg_walk_aim_adopt, dim3(1, walkers), dim3(BLOCK), 0, stream, d_bases, d_gen,
                       d_consts, n_leaves, seed, r, lanes, max_rounds, d_entries, n_entries,
                       d_pieces, d_resid, n_resid, d_rstate, d_lives, d_state, d_trace);
    return hipGetLastError();
}

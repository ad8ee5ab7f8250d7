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
// Thread 0 applies the adopted lane under the OLD side rows, before the
// barrier; the block replaces them after it, as it replaces the residual
// values.  Before round 0's adoption no entry is live and nothing is read.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_walk_sum.h"
#include "mg_walk_tree.h"

#define BLOCK 256
// blocks per walker and launch: tiles beyond are grid-strided (as mg_walk.hip)
#define MAX_BLOCKS 2048u

static_assert(MG_AIM_MAX_ENTRIES <= BLOCK, "one thread per entry builds the live list");
static_assert(MG_UF_MAX_SLOTS <= BLOCK, "one thread per slot resolves it");

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
    __shared__ uint32_t s_lane;                  // the adopted lane, or MG_AIM_NONE
    __shared__ uint32_t s_flag[BLOCK];
    __shared__ uint32_t s_dest[MG_UF_MAX_SLOTS];
    const uint32_t w = blockIdx.y;
    const size_t total = (size_t)gridDim.y * lanes;
    uint32_t* base = bases + (size_t)w * n_leaves * 8;
    uint32_t* rvals = rstate + (size_t)w * n_resid * 8;
    uint32_t* mvals = mstate + (size_t)w * n_mwords;
    uint32_t* svals = sstate + (size_t)w * n_srows * 8;
    uint32_t* uvals = ustate + (size_t)w * n_urows * 8;
    uint32_t* dest = dests + (size_t)w * n_slots;
    uint32_t* live = lives + (size_t)w * MG_AIM_LIVE_WORDS;
    if (threadIdx.x == 0) {
        const unsigned long long key = st[w].key;
        const uint32_t nfail = (uint32_t)(key >> MG_WALK_NFAIL_SHIFT);
        const uint32_t cost = (uint32_t)(key >> MG_WALK_COST_SHIFT) & MG_WALK_FIELD;
        const uint32_t j = (uint32_t)key & MG_WALK_FIELD;
        const bool better = nfail < st[w].nfail || (nfail == st[w].nfail && cost < st[w].cost);
        const bool adopt = key != ~0ull && better && j < lanes;
        if (adopt) {
            // the moves and the gathered side are computed from the base
            // before anything is stored; the old residual values, side rows,
            // live list and destinations are read here, before the barrier,
            // and replaced after it
            mg_walk_sum_lane(base, gen, consts, n_leaves, mg_walk_seed(seed, w), r, j, lanes,
                             entries, pieces, fixed, lin, rvals, svals, live, dest, base, 1,
                             nullptr);
            st[w].nfail = nfail;
            st[w].cost = cost;
        }
        trace[((size_t)w * max_rounds + r) * 2] = nfail;
        trace[((size_t)w * max_rounds + r) * 2 + 1] = cost;
        st[w].key = ~0ull;
        s_lane = adopt ? j : MG_AIM_NONE;
    }
    __syncthreads();                             // the new base is visible to the block
    const uint32_t j = s_lane;                                             // block-uniform
    if (j == MG_AIM_NONE) return;
    const uint32_t* column = resid + (size_t)w * lanes + j;
    const uint32_t* mcolumn = masks + (size_t)w * lanes + j;
    const uint32_t* scolumn = srows + (size_t)w * lanes + j;
    const uint32_t* ucolumn = urows + (size_t)w * lanes + j;
    for (uint32_t i = threadIdx.x; i < n_resid * 8; i += BLOCK) rvals[i] = column[(size_t)i * total];
    for (uint32_t i = threadIdx.x; i < n_mwords; i += BLOCK) mvals[i] = mcolumn[(size_t)i * total];
    for (uint32_t i = threadIdx.x; i < n_srows * 8; i += BLOCK) svals[i] = scolumn[(size_t)i * total];
    for (uint32_t i = threadIdx.x; i < n_urows * 8; i += BLOCK) uvals[i] = ucolumn[(size_t)i * total];
    const uint32_t e = threadIdx.x;
    if (e < n_slots) {
        const uint32_t d = mg_walk_uf_resolve(slots, funcs, cands, ukeys, e, base, ucolumn, total);
        s_dest[e] = d;
        dest[e] = d;
    }
    __syncthreads();
    s_flag[e] = e < n_entries && mg_walk_uf_is_live(entries, pieces, e, column, mcolumn, n_rwords,
                                                    total, s_dest) ? 1u : 0u;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t i = 0; i < BLOCK; ++i) before += i < e ? s_flag[i] : 0u;
    if (s_flag[e]) live[1 + before] = e;
    if (e == BLOCK - 1) live[0] = before + s_flag[e];
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

/* The round of the aimed walks on the device, hipcc
 * only: the block size and grid of every tree-scored walk's kernels, and the
 * three bodies of the round that mg_walk_bound, mg_walk_uf, mg_walk_sum and
 * mg_walk_batch share,
 *   mg_walk_mutate_body  lane j of walker w writes neighbour j of base w (the
 *                        lane function of mg_walk_sum.h)
 *   mg_walk_score_body   lane j scores neighbour j (mg_walk_tree.h); walker
 *                        w's key is the minimum over its lanes
 *   mg_walk_adopt_body   block w adopts walker w's best neighbour and rebuilds
 *                        the walker's state from that lane's probes
 * The kernels of mg_walk_sum.hip, mg_walk_tree.hip and mg_walk_batch.hip only
 * unpack their arguments and call a body.
 *
 * The bodies take what the single walk's kernels take, as __restrict__
 * parameters: a batch's pointers are loaded from memory, and without the
 * promise the compiler must reload the base and the tables after every store
 * of a neighbour (a one-job batch took 0.072 ms per round without it and
 * 0.050 ms with it, beside the single walk's 0.045 ms). */
#ifndef MG_WALK_ROUND_H
#define MG_WALK_ROUND_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_walk_sum.h"
#include "mg_walk_tree.h"

#define MG_WALK_BLOCK 256
/* blocks per walker and launch: tiles beyond are grid-strided (as mg_walk.hip) */
#define MG_WALK_MAX_BLOCKS 2048u
#define MG_WALK_TILES(lanes) (((lanes) + MG_WALK_BLOCK - 1) / MG_WALK_BLOCK)

static_assert(MG_AIM_MAX_ENTRIES <= MG_WALK_BLOCK, "one thread per entry builds the live list");
static_assert(MG_UF_MAX_SLOTS <= MG_WALK_BLOCK, "one thread per slot resolves it");

/* the x extent of a mutate or score grid over `lanes` lanes per walker */
static inline uint32_t mg_walk_grid_blocks(uint32_t lanes) {
    const uint32_t tiles = MG_WALK_TILES(lanes);
    return tiles < MG_WALK_MAX_BLOCKS ? tiles : MG_WALK_MAX_BLOCKS;
}

/* the score kernel of every tree-scored walk (mg_walk_tree.hip) */
__global__ __launch_bounds__(MG_WALK_BLOCK) void mg_walk_tree_score(
    const uint32_t* __restrict__ masks, const uint32_t* __restrict__ amasks,
    const uint32_t* __restrict__ resid, const uint32_t* __restrict__ roots,
    const uint32_t* __restrict__ atoms, const uint32_t* __restrict__ code, uint32_t lanes,
    uint32_t n_roots, mg_walk_state* __restrict__ st);

/* Grid (blocks, walkers[, jobs]).  rstate: [walkers][n_resid][8], sstate:
 * [walkers][n_srows][8], lives: [walkers][MG_AIM_LIVE_WORDS], dests: [walkers]
 * [n_slots]; out: the interpreter's eval-mode input. */
static __device__ __forceinline__ void mg_walk_mutate_body(
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
    const uint32_t tiles = MG_WALK_TILES(lanes);
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // uniform per block
        const uint32_t j = tile * MG_WALK_BLOCK + threadIdx.x;
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

/* Grid (blocks, walkers[, jobs]).  The stack of the postfix programs lives in
 * LDS (mg_walk_tree.hip says why). */
static __device__ __forceinline__ void mg_walk_score_body(
    const uint32_t* __restrict__ masks, const uint32_t* __restrict__ amasks,
    const uint32_t* __restrict__ resid, const uint32_t* __restrict__ roots,
    const uint32_t* __restrict__ atoms, const uint32_t* __restrict__ code, uint32_t lanes,
    uint32_t n_roots, mg_walk_state* __restrict__ st) {
    __shared__ unsigned long long s_best;
    __shared__ uint32_t s_stack[MG_WT_STACK * MG_WALK_BLOCK];
    if (threadIdx.x == 0) s_best = ~0ull;
    __syncthreads();
    const uint32_t w = blockIdx.y;
    const size_t total = (size_t)gridDim.y * lanes;
    const uint32_t tiles = MG_WALK_TILES(lanes);
    unsigned long long best = ~0ull;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // uniform per block
        const uint32_t j = tile * MG_WALK_BLOCK + threadIdx.x;
        // lanes past the walker's stay in the loop (the wave-wide OR and the
        // wave-uniform programs need the whole wave) and read nothing
        const bool active = j < lanes;
        uint32_t nfail, cost;
        mg_walk_tree_score_lane(masks, amasks, resid, total, (size_t)w * lanes + (active ? j : 0u),
                                roots, atoms, code, n_roots, active, s_stack + threadIdx.x,
                                MG_WALK_BLOCK, &nfail, &cost);
        const unsigned long long key = active ? mg_walk_key(nfail, cost, j) : ~0ull;
        best = key < best ? key : best;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o < best ? o : best;
    }
    if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(&s_best, best);
    __syncthreads();
    if (threadIdx.x == 0 && s_best != ~0ull) atomicMin(&st[w].key, s_best);
}

/* The adoption of walker w, by one block of MG_WALK_BLOCK threads
 * (mg_walk_sum.hip says what it does).  total: the lanes of all walkers, the
 * row stride of the probe buffer.  masks: the root mask rows, then the atom
 * mask rows (n_mwords words per lane, the first n_rwords the root mask's);
 * srows: the n_srows probes after the residuals, urows: the n_urows probes
 * after them; mstate: [walkers][n_mwords], ustate: [walkers][n_urows][8]. */
static __device__ __forceinline__ void mg_walk_adopt_body(
    uint32_t w, size_t total, uint32_t* bases, const mg_leafgen* __restrict__ gen,
    const uint32_t* __restrict__ consts, uint32_t n_leaves, uint64_t seed, uint32_t r,
    uint32_t lanes, uint32_t max_rounds, const uint32_t* __restrict__ entries, uint32_t n_entries,
    const uint32_t* __restrict__ pieces, const uint32_t* __restrict__ fixed,
    const uint32_t* __restrict__ lin, const uint32_t* __restrict__ resid, uint32_t n_resid,
    const uint32_t* __restrict__ masks, uint32_t n_mwords, uint32_t n_rwords,
    const uint32_t* __restrict__ srows, uint32_t n_srows, uint32_t* sstate,
    const uint32_t* __restrict__ urows, uint32_t n_urows, const uint32_t* __restrict__ slots,
    uint32_t n_slots, const uint32_t* __restrict__ funcs, const uint32_t* __restrict__ cands,
    const uint32_t* __restrict__ ukeys, uint32_t* rstate, uint32_t* mstate, uint32_t* ustate,
    uint32_t* dests, uint32_t* lives, mg_walk_state* __restrict__ st,
    uint32_t* __restrict__ trace) {
    __shared__ uint32_t s_lane;                  // the adopted lane, or MG_AIM_NONE
    __shared__ uint32_t s_flag[MG_WALK_BLOCK];
    __shared__ uint32_t s_dest[MG_UF_MAX_SLOTS];
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
    for (uint32_t i = threadIdx.x; i < n_resid * 8; i += MG_WALK_BLOCK)
        rvals[i] = column[(size_t)i * total];
    for (uint32_t i = threadIdx.x; i < n_mwords; i += MG_WALK_BLOCK)
        mvals[i] = mcolumn[(size_t)i * total];
    for (uint32_t i = threadIdx.x; i < n_srows * 8; i += MG_WALK_BLOCK)
        svals[i] = scolumn[(size_t)i * total];
    for (uint32_t i = threadIdx.x; i < n_urows * 8; i += MG_WALK_BLOCK)
        uvals[i] = ucolumn[(size_t)i * total];
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
    for (uint32_t i = 0; i < MG_WALK_BLOCK; ++i) before += i < e ? s_flag[i] : 0u;
    if (s_flag[e]) live[1 + before] = e;
    if (e == MG_WALK_BLOCK - 1) live[0] = before + s_flag[e];
}

#endif

// mg_walk — several greedy walkers per launch, neighbours ranked by (failing
// roots, distance inside the failing roots) (specification:
// mythril_amd/repair.py walk_ref).
//
// One round = four launches on the context stream, no host round trip; every
// launch covers all walkers (grid.y = walker, so no wave spans two walkers):
//   mg_walk_mutate   lane j of walker w writes neighbour j of base w (the move
//                    function of mg_repair.h under the seed of walker w) as
//                    the interpreter's eval-mode input [leaf][limb][W * lanes],
//                    walker w in columns w * lanes ..
//   the interpreter  (eval mode) writes every neighbour's verdict mask and
//                    residual probes
//   mg_walk_score    lane j scores neighbour j (mg_walk.h); walker w's key is
//                    min over its lanes of nfail << 40 | cost << 20 | lane
//   mg_walk_adopt    thread w: a neighbour with a strictly smaller (nfail,
//                    cost) than base w becomes base w (recomputed from its
//                    lane number: no gather); the round's best (nfail, cost)
//                    goes to the trace, the key is reset
// Lane 0 is the base itself, so round 0 measures the start and a base's key
// never rises.  Sums and minima only: the result does not depend on the
// order of blocks.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_walk.h"

#define BLOCK 256
// blocks per walker and launch: tiles beyond are grid-strided
#define MAX_BLOCKS 2048u

__global__ __launch_bounds__(BLOCK) void mg_walk_mutate(
    const uint32_t* __restrict__ bases, const mg_leafgen* __restrict__ gen,
    const uint32_t* __restrict__ consts, uint32_t n_leaves, uint64_t seed, uint32_t r,
    uint32_t lanes, uint32_t* __restrict__ out) {
    const uint32_t w = blockIdx.y;
    const size_t total = (size_t)gridDim.y * lanes;
    const uint32_t* base = bases + (size_t)w * n_leaves * 8;
    const uint64_t wseed = mg_walk_seed(seed, w);
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // uniform per block
        const uint32_t j = tile * BLOCK + threadIdx.x;
        if (j >= lanes) continue;
        mg_repair_moves mv;
        mg_repair_lane(base, gen, consts, n_leaves, wseed, r, j, lanes, &mv);
        const bool m0 = mv.n > 0, m1 = mv.n > 1;
        const size_t col = (size_t)w * lanes + j;
        for (uint32_t leaf = 0; leaf < n_leaves; ++leaf) {
            const bool t0 = m0 && mv.leaf[0] == leaf, t1 = m1 && mv.leaf[1] == leaf;
            for (uint32_t k = 0; k < 8; ++k) {
                const uint32_t b = base[(size_t)leaf * 8 + k];            // wave-uniform
                const uint32_t v = t1 ? mv.val[1][k] : (t0 ? mv.val[0][k] : b);
                out[((size_t)leaf * 8 + k) * total + col] = v;            // one row: coalesced
            }
        }
    }
}

__global__ __launch_bounds__(BLOCK) void mg_walk_score(
    const uint32_t* __restrict__ masks, const uint32_t* __restrict__ resid,
    const uint32_t* __restrict__ table, uint32_t lanes, uint32_t n_roots,
    mg_walk_state* __restrict__ st) {
    __shared__ unsigned long long s_best;
    if (threadIdx.x == 0) s_best = ~0ull;
    __syncthreads();
    const uint32_t w = blockIdx.y;
    const size_t total = (size_t)gridDim.y * lanes;
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    unsigned long long best = ~0ull;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // uniform per block
        const uint32_t j = tile * BLOCK + threadIdx.x;
        // lanes past the walker's stay in the loop (the wave-wide OR of
        // mg_walk_score_lane needs the whole wave) and read nothing
        const bool active = j < lanes;
        uint32_t nfail, cost;
        mg_walk_score_lane(masks, resid, total, (size_t)w * lanes + (active ? j : 0u), table,
                           n_roots, active, &nfail, &cost);
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

__global__ __launch_bounds__(64) void mg_walk_adopt(
    uint32_t* __restrict__ bases, const mg_leafgen* __restrict__ gen,
    const uint32_t* __restrict__ consts, uint32_t n_leaves, uint64_t seed, uint32_t r,
    uint32_t lanes, uint32_t walkers, uint32_t max_rounds, mg_walk_state* __restrict__ st,
    uint32_t* __restrict__ trace) {
    const uint32_t w = blockIdx.x * 64 + threadIdx.x;
    if (w >= walkers) return;
    uint32_t* base = bases + (size_t)w * n_leaves * 8;
    const unsigned long long key = st[w].key;
    const uint32_t nfail = (uint32_t)(key >> MG_WALK_NFAIL_SHIFT);
    const uint32_t cost = (uint32_t)(key >> MG_WALK_COST_SHIFT) & MG_WALK_FIELD;
    const uint32_t j = (uint32_t)key & MG_WALK_FIELD;
    const bool better = nfail < st[w].nfail || (nfail == st[w].nfail && cost < st[w].cost);
    if (key != ~0ull && better && j < lanes) {
        // every read of the base happens in mg_repair_lane, before the stores
        mg_repair_moves mv;
        mg_repair_lane(base, gen, consts, n_leaves, mg_walk_seed(seed, w), r, j, lanes, &mv);
        for (uint32_t m = 0; m < mv.n; ++m)
            for (uint32_t k = 0; k < 8; ++k) base[(size_t)mv.leaf[m] * 8 + k] = mv.val[m][k];
        st[w].nfail = nfail;
        st[w].cost = cost;
    }
    trace[((size_t)w * max_rounds + r) * 2] = nfail;
    trace[((size_t)w * max_rounds + r) * 2 + 1] = cost;
    st[w].key = ~0ull;
}

static bool walk_shape_ok(uint32_t walkers, uint32_t lanes, uint32_t n_leaves, uint32_t r) {
    return walkers >= 1 && walkers <= MG_WALK_MAX_WALKERS && lanes >= 1 &&
           lanes <= MG_REPAIR_MAX_LANES && n_leaves > 0 && r < MG_REPAIR_MAX_ROUNDS;
}

hipError_t mg_launch_walk_round(const uint32_t* d_bases, const mg_leafgen* d_gen,
                                const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                                uint32_t r, uint32_t lanes, uint32_t walkers, uint32_t* d_leaves,
                                hipStream_t stream) {
    if (!walk_shape_ok(walkers, lanes, n_leaves, r)) return hipErrorInvalidValue;
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    const uint32_t blocks = tiles < MAX_BLOCKS ? tiles : MAX_BLOCKS;
    hipLaunchKernelGGL(mg_walk_mutate, dim3(blocks, walkers), dim3(BLOCK), 0, stream, d_bases,
                       d_gen, d_consts, n_leaves, seed, r, lanes, d_leaves);
    return hipGetLastError();
}

hipError_t mg_launch_walk_pick(const uint32_t* d_masks, const uint32_t* d_resid,
                               const uint32_t* d_table, uint32_t lanes, uint32_t walkers,
                               uint32_t n_roots, uint32_t* d_bases, const mg_leafgen* d_gen,
                               const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                               uint32_t r, uint32_t max_rounds, mg_walk_state* d_state,
                               uint32_t* d_trace, hipStream_t stream) {
    if (!walk_shape_ok(walkers, lanes, n_leaves, r) || n_roots == 0 || n_roots > 1024 ||
        r >= max_rounds)
        return hipErrorInvalidValue;
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    const uint32_t blocks = tiles < MAX_BLOCKS ? tiles : MAX_BLOCKS;
    hipLaunchKernelGGL(mg_walk_score, dim3(blocks, walkers), dim3(BLOCK), 0, stream, d_masks,
                       d_resid, d_table, lanes, n_roots, d_state);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mg_walk_adopt, dim3((walkers + 63) / 64), dim3(64), 0, stream, d_bases,
                       d_gen, d_consts, n_leaves, seed, r, lanes, walkers, max_rounds, d_state,
                       d_trace);
    return hipGetLastError();
}

// the adopt step alone, for a round that scores with another kernel
// (mg_walk_tree.hip)
hipError_t mg_launch_walk_adopt(uint32_t* d_bases, const mg_leafgen* d_gen,
                                const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                                uint32_t r, uint32_t lanes, uint32_t walkers, uint32_t max_rounds,
                                mg_walk_state* d_state, uint32_t* d_trace, hipStream_t stream) {
    if (!walk_shape_ok(walkers, lanes, n_leaves, r) || r >= max_rounds)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mg_walk_adopt, dim3((walkers + 63) / 64), dim3(64), 0, stream, d_bases,
                       d_gen, d_consts, n_leaves, seed, r, lanes, walkers, max_rounds, d_state,
                       d_trace);
    return hipGetLastError();
}

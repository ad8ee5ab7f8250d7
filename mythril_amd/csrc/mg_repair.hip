// mg_repair — greedy local search from a nearly satisfying candidate
// (specification: mythril_amd/repair.py repair_ref).
//
// One round = four launches on the context stream, no host round trip:
//   mg_repair_mutate  lane j writes neighbour j of the base assignment (the
//                     move function of mg_repair.h) as the interpreter's
//                     eval-mode input, [leaf][limb][lane] u32
//   the interpreter   (eval mode) writes every neighbour's verdict mask as
//                     probes, as for the census (mg_census.hip)
//   mg_repair_select  lane j counts neighbour j's failing roots; the round's
//                     key is min over lanes of nfail << 32 | lane
//   mg_repair_adopt   a neighbour strictly better than the base becomes the
//                     base (recomputed from its lane number: no gather); the
//                     round's best count goes to the trace, the key is reset
// Lane 0 is the base itself, so round 0 measures the start and the base's
// count never rises.  Minima only: the result does not depend on the order
// of blocks.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_repair.h"

#define BLOCK 256
// blocks per launch: 8 per CU of a 256-CU part; tiles beyond are grid-strided
#define MAX_BLOCKS 2048u

__global__ __launch_bounds__(BLOCK) void mg_repair_mutate(
    const uint32_t* __restrict__ base, const mg_leafgen* __restrict__ gen,
    const uint32_t* __restrict__ consts, uint32_t n_leaves, uint64_t seed, uint32_t r,
    uint32_t lanes, uint32_t* __restrict__ out) {
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // uniform per block
        const uint32_t j = tile * BLOCK + threadIdx.x;
        if (j >= lanes) continue;
        // the move reads one leaf's descriptor and value per lane (a gather
        // of a few dwords); the rows below read the base uniformly
        mg_repair_moves mv;
        mg_repair_lane(base, gen, consts, n_leaves, seed, r, j, lanes, &mv);
        const bool m0 = mv.n > 0, m1 = mv.n > 1;
        for (uint32_t leaf = 0; leaf < n_leaves; ++leaf) {
            const bool t0 = m0 && mv.leaf[0] == leaf, t1 = m1 && mv.leaf[1] == leaf;
            for (uint32_t k = 0; k < 8; ++k) {
                const uint32_t b = base[(size_t)leaf * 8 + k];            // wave-uniform
                const uint32_t v = t1 ? mv.val[1][k] : (t0 ? mv.val[0][k] : b);
                out[((size_t)leaf * 8 + k) * lanes + j] = v;              // one row: coalesced
            }
        }
    }
}

__global__ __launch_bounds__(BLOCK) void mg_repair_select(
    const uint32_t* __restrict__ rows, uint32_t lanes, uint32_t n_roots,
    mg_repair_state* __restrict__ st) {
    __shared__ unsigned long long s_best;
    if (threadIdx.x == 0) s_best = ~0ull;
    __syncthreads();
    const uint32_t n_words = (n_roots + 31) / 32;
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    unsigned long long best = ~0ull;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t j = tile * BLOCK + threadIdx.x;
        if (j >= lanes) continue;               // lanes past the round: the interpreter wrote nothing
        uint32_t nfail = 0;
        for (uint32_t q = 0; q < n_words; ++q) {
            const uint32_t bits = n_roots - 32 * q < 32 ? n_roots - 32 * q : 32;
            const uint32_t valid = bits == 32 ? ~0u : (1u << bits) - 1u;   // bits >= n_roots: ignored
            nfail += __builtin_popcount(~rows[(size_t)q * lanes + j] & valid);
        }
        const unsigned long long key = ((unsigned long long)nfail << 32) | j;
        best = key < best ? key : best;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o < best ? o : best;
    }
    if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(&s_best, best);
    __syncthreads();
    if (threadIdx.x == 0 && s_best != ~0ull) atomicMin(&st->key, s_best);
}

__global__ __launch_bounds__(64) void mg_repair_adopt(
    uint32_t* __restrict__ base, const mg_leafgen* __restrict__ gen,
    const uint32_t* __restrict__ consts, uint32_t n_leaves, uint64_t seed, uint32_t r,
    uint32_t lanes, mg_repair_state* __restrict__ st, uint32_t* __restrict__ trace) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long key = st->key;
    const uint32_t nfail = (uint32_t)(key >> 32), j = (uint32_t)key;
    if (key != ~0ull && nfail < st->base_nfail && j < lanes) {
        // every read of the base happens in mg_repair_lane, before the stores
        mg_repair_moves mv;
        mg_repair_lane(base, gen, consts, n_leaves, seed, r, j, lanes, &mv);
        for (uint32_t m = 0; m < mv.n; ++m)
            for (uint32_t k = 0; k < 8; ++k) base[(size_t)mv.leaf[m] * 8 + k] = mv.val[m][k];
        st->base_nfail = nfail;
    }
    trace[r] = nfail;
    st->rounds = r + 1;
    st->key = ~0ull;
}

hipError_t mg_launch_repair_round(uint32_t* d_base, const mg_leafgen* d_gen,
                                  const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                                  uint32_t r, uint32_t lanes, uint32_t* d_leaves,
                                  hipStream_t stream) {
    if (lanes == 0 || lanes > MG_REPAIR_MAX_LANES || n_leaves == 0 || r >= MG_REPAIR_MAX_ROUNDS)
        return hipErrorInvalidValue;
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    const uint32_t blocks = tiles < MAX_BLOCKS ? tiles : MAX_BLOCKS;
    hipLaunchKernelGGL(mg_repair_mutate, dim3(blocks), dim3(BLOCK), 0, stream, d_base, d_gen,
                       d_consts, n_leaves, seed, r, lanes, d_leaves);
    return hipGetLastError();
}

hipError_t mg_launch_repair_pick(const uint32_t* d_rows, uint32_t lanes, uint32_t n_roots,
                                 uint32_t* d_base, const mg_leafgen* d_gen,
                                 const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                                 uint32_t r, mg_repair_state* d_state, uint32_t* d_trace,
                                 hipStream_t stream) {
    if (lanes == 0 || lanes > MG_REPAIR_MAX_LANES || n_leaves == 0 || n_roots == 0 ||
        n_roots > 1024 || r >= MG_REPAIR_MAX_ROUNDS)
        return hipErrorInvalidValue;
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    const uint32_t blocks = tiles < MAX_BLOCKS ? tiles : MAX_BLOCKS;
    hipLaunchKernelGGL(mg_repair_select, dim3(blocks), dim3(BLOCK), 0, stream, d_rows, lanes,
                       n_roots, d_state);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mg_repair_adopt, dim3(1), dim3(64), 0, stream, d_base, d_gen, d_consts,
                       n_leaves, seed, r, lanes, d_state, d_trace);
    return hipGetLastError();
}

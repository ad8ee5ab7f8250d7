// mg_walk_batch — the tree-scored walks of several groups in one launch
// sequence.  One walker at 4096 lanes is 16 blocks, a
// sixteenth of the device; the walks of different groups do not depend on
// each other, so a batch runs the round of mg_walk_sum.hip with a job axis:
//   mg_walk_batch_mutate  grid (blocks, walkers, jobs): mg_walk_sum_mutate
//   the interpreter       grid (tiles, jobs): one launch over the batch's
//                         descriptors; job g reads its leaves and writes its
//                         probes at g times the batch's strides (the shell's
//                         leaves_prog_words / probe_prog_words) and returns at
//                         once when its skip_prog word is set
//   mg_walk_batch_score   grid (blocks, walkers, jobs): mg_walk_tree_score
//   mg_walk_batch_adopt   grid (1, walkers, jobs): mg_walk_sum_adopt
// blockIdx.z selects a device-resident mg_walk_batch_job (mg_walk_batch.h):
// the pointers and counts the single walk's kernels take as arguments.  The
// lane-level work is the single walk's own (mg_walk_sum_lane,
// mg_walk_tree_score_lane, mg_walk_uf_resolve, mg_walk_uf_is_live, and the
// adopt body both adopt kernels call), so job g's outputs are those of
// mg_walk_sum on it alone, bit for bit.
// Freeze rule: frozen[g] != 0 (the interpreter's skip_prog array) makes every
// block of job g return before it reads the job.  The host sets it at the
// sync point where the single walk of g would have stopped; nothing of the
// job is written afterwards, so its trace rows past the stop stay zero.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_walk_batch.h"

#define BLOCK MG_WALK_BLOCK
// blocks per walker and launch: tiles beyond are grid-strided (as mg_walk.hip)
#define MAX_BLOCKS 2048u

// The bodies take what the single walk's kernels take, as __restrict__
// parameters: the job's pointers are loaded from memory, and without the
// promise the compiler must reload the base and the tables after every store
// of a neighbour (a one-job batch took 0.072 ms per round without it and
// 0.050 ms with it, beside the single walk's 0.045 ms).
static __device__ __forceinline__ void mutate_body(
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

__global__ __launch_bounds__(BLOCK) void mg_walk_batch_mutate(
    const mg_walk_batch_job* __restrict__ jobs, const uint32_t* __restrict__ frozen, uint32_t r,
    uint32_t lanes) {
    if (frozen[blockIdx.z]) return;                                        // block-uniform
    const mg_walk_batch_job* J = jobs + blockIdx.z;
    mutate_body(J->bases, J->gen, J->consts, J->n_leaves, J->seed, r, lanes, J->entries,
                J->pieces, J->fixed, J->lin, J->rstate, J->n_resid, J->sstate, J->n_srows,
                J->lives, J->dests, J->n_slots, J->leaves);
}

// the body of mg_walk_tree_score (mg_walk_tree.hip): the stack of the postfix
// programs in LDS
static __device__ __forceinline__ void score_body(
    const uint32_t* __restrict__ masks, const uint32_t* __restrict__ amasks,
    const uint32_t* __restrict__ resid, const uint32_t* __restrict__ roots,
    const uint32_t* __restrict__ atoms, const uint32_t* __restrict__ code, uint32_t lanes,
    uint32_t n_roots, mg_walk_state* __restrict__ st) {
    __shared__ unsigned long long s_best;
    __shared__ uint32_t s_stack[MG_WT_STACK * BLOCK];
    if (threadIdx.x == 0) s_best = ~0ull;
    __syncthreads();
    const uint32_t w = blockIdx.y;
    const size_t total = (size_t)gridDim.y * lanes;
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    unsigned long long best = ~0ull;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // uniform per block
        const uint32_t j = tile * BLOCK + threadIdx.x;
        // lanes past the walker's stay in the loop (the wave-wide OR and the
        // wave-uniform programs need the whole wave) and read nothing
        const bool active = j < lanes;
        uint32_t nfail, cost;
        mg_walk_tree_score_lane(masks, amasks, resid, total, (size_t)w * lanes + (active ? j : 0u),
                                roots, atoms, code, n_roots, active, s_stack + threadIdx.x, BLOCK,
                                &nfail, &cost);
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

__global__ __launch_bounds__(BLOCK) void mg_walk_batch_score(
    const mg_walk_batch_job* __restrict__ jobs, const uint32_t* __restrict__ frozen,
    uint32_t lanes) {
    if (frozen[blockIdx.z]) return;                                        // block-uniform
    const mg_walk_batch_job* J = jobs + blockIdx.z;
    score_body(J->masks, J->amasks, J->resid, J->roots, J->atoms, J->code, lanes, J->n_roots,
               J->state);
}

__global__ __launch_bounds__(BLOCK) void mg_walk_batch_adopt(
    const mg_walk_batch_job* __restrict__ jobs, const uint32_t* __restrict__ frozen, uint32_t r,
    uint32_t lanes, uint32_t max_rounds) {
    if (frozen[blockIdx.z]) return;                                        // block-uniform
    const mg_walk_batch_job* J = jobs + blockIdx.z;
    const uint32_t n_rwords = MG_BOUND_MASK_WORDS(J->n_roots),
                   n_mwords = n_rwords + MG_BOUND_MASK_WORDS(J->n_atoms);
    mg_walk_sum_adopt_body(blockIdx.y, (size_t)gridDim.y * lanes, J->bases, J->gen, J->consts,
                           J->n_leaves, J->seed, r, lanes, max_rounds, J->entries, J->n_entries,
                           J->pieces, J->fixed, J->lin, J->resid, J->n_resid, J->masks, n_mwords,
                           n_rwords, J->srows, J->n_srows, J->sstate, J->urows, J->n_urows,
                           J->slots, J->n_slots, J->funcs, J->cands, J->ukeys, J->rstate,
                           J->mstate, J->ustate, J->dests, J->lives, J->state, J->trace);
}

static bool batch_shape_ok(uint32_t n_jobs, uint32_t walkers, uint32_t lanes, uint32_t r,
                           uint32_t max_rounds) {
    return mg_walk_batch_shared_ok(n_jobs, walkers, lanes, max_rounds) && r < max_rounds;
}

// Every job must have passed what mg_walk_sum checks (mg_walk_batch does that
// before it uploads).  d_frozen: [n_jobs], the interpreter's skip_prog too.
hipError_t mg_launch_walk_batch_round(const mg_walk_batch_job* d_jobs, const uint32_t* d_frozen,
                                     uint32_t n_jobs, uint32_t r, uint32_t lanes,
                                     uint32_t walkers, uint32_t max_rounds, hipStream_t stream) {
    if (!batch_shape_ok(n_jobs, walkers, lanes, r, max_rounds)) return hipErrorInvalidValue;
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    const uint32_t blocks = tiles < MAX_BLOCKS ? tiles : MAX_BLOCKS;
    hipLaunchKernelGGL(mg_walk_batch_mutate, dim3(blocks, walkers, n_jobs), dim3(BLOCK), 0, stream,
                       d_jobs, d_frozen, r, lanes);
    return hipGetLastError();
}

// score, then adopt, after the interpreter wrote every job's probes
hipError_t mg_launch_walk_batch_pick(const mg_walk_batch_job* d_jobs, const uint32_t* d_frozen,
                                    uint32_t n_jobs, uint32_t r, uint32_t lanes, uint32_t walkers,
                                    uint32_t max_rounds, hipStream_t stream) {
    if (!batch_shape_ok(n_jobs, walkers, lanes, r, max_rounds)) return hipErrorInvalidValue;
    const uint32_t tiles = (lanes + BLOCK - 1) / BLOCK;
    const uint32_t blocks = tiles < MAX_BLOCKS ? tiles : MAX_BLOCKS;
    hipLaunchKernelGGL(mg_walk_batch_score, dim3(blocks, walkers, n_jobs), dim3(BLOCK), 0, stream,
                       d_jobs, d_frozen, lanes);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mg_walk_batch_adopt, dim3(1, walkers, n_jobs), dim3(BLOCK), 0, stream,
                       d_jobs, d_frozen, r, lanes, max_rounds);
    return hipGetLastError();
}

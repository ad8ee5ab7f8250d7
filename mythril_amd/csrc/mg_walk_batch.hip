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
// work is the single walk's own (the three bodies of mg_walk_round.h, which
// the single walk's kernels call too), so job g's outputs are those of
// mg_walk_sum on it alone, bit for bit.
// Freeze rule: frozen[g] != 0 (the interpreter's skip_prog array) makes every
// block of job g return before it reads the job.  The host sets it at the
// sync point where the single walk of g would have stopped; nothing of the
// job is written afterwards, so its trace rows past the stop stay zero.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_walk_batch.h"
#include "mg_walk_round.h"

__global__ __launch_bounds__(MG_WALK_BLOCK) void mg_walk_batch_mutate(
    const mg_walk_batch_job* __restrict__ jobs, const uint32_t* __restrict__ frozen, uint32_t r,
    uint32_t lanes) {
    if (frozen[blockIdx.z]) return;                                        // block-uniform
    const mg_walk_batch_job* J = jobs + blockIdx.z;
    mg_walk_mutate_body(J->bases, J->gen, J->consts, J->n_leaves, J->seed, r, lanes, J->entries,
                        J->pieces, J->fixed, J->lin, J->rstate, J->n_resid, J->sstate,
                        J->n_srows, J->lives, J->dests, J->n_slots, J->leaves);
}

__global__ __launch_bounds__(MG_WALK_BLOCK) void mg_walk_batch_score(
    const mg_walk_batch_job* __restrict__ jobs, const uint32_t* __restrict__ frozen,
    uint32_t lanes) {
    if (frozen[blockIdx.z]) return;                                        // block-uniform
    const mg_walk_batch_job* J = jobs + blockIdx.z;
    mg_walk_score_body(J->masks, J->amasks, J->resid, J->roots, J->atoms, J->code, lanes,
                       J->n_roots, J->state);
}

__global__ __launch_bounds__(MG_WALK_BLOCK) void mg_walk_batch_adopt(
    const mg_walk_batch_job* __restrict__ jobs, const uint32_t* __restrict__ frozen, uint32_t r,
    uint32_t lanes, uint32_t max_rounds) {
    if (frozen[blockIdx.z]) return;                                        // block-uniform
    const mg_walk_batch_job* J = jobs + blockIdx.z;
    const uint32_t n_rwords = MG_BOUND_MASK_WORDS(J->n_roots),
                   n_mwords = n_rwords + MG_BOUND_MASK_WORDS(J->n_atoms);
    mg_walk_adopt_body(blockIdx.y, (size_t)gridDim.y * lanes, J->bases, J->gen, J->consts,
                       J->n_leaves, J->seed, r, lanes, max_rounds, J->entries, J->n_entries,
                       J->pieces, J->fixed, J->lin, J->resid, J->n_resid, J->masks, n_mwords,
                       n_rwords, J->srows, J->n_srows, J->sstate, J->urows, J->n_urows, J->slots,
                       J->n_slots, J->funcs, J->cands, J->ukeys, J->rstate, J->mstate, J->ustate,
                       J->dests, J->lives, J->state, J->trace);
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
    const uint32_t blocks = mg_walk_grid_blocks(lanes);
    hipLaunchKernelGGL(mg_walk_batch_mutate, dim3(blocks, walkers, n_jobs), dim3(MG_WALK_BLOCK), 0,
                       stream, d_jobs, d_frozen, r, lanes);
    return hipGetLastError();
}

// score, then adopt, after the interpreter wrote every job's probes
hipError_t mg_launch_walk_batch_pick(const mg_walk_batch_job* d_jobs, const uint32_t* d_frozen,
                                    uint32_t n_jobs, uint32_t r, uint32_t lanes, uint32_t walkers,
                                    uint32_t max_rounds, hipStream_t stream) {
    if (!batch_shape_ok(n_jobs, walkers, lanes, r, max_rounds)) return hipErrorInvalidValue;
    const uint32_t blocks = mg_walk_grid_blocks(lanes);
    hipLaunchKernelGGL(mg_walk_batch_score, dim3(blocks, walkers, n_jobs), dim3(MG_WALK_BLOCK), 0,
                       stream, d_jobs, d_frozen, lanes);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mg_walk_batch_adopt, dim3(1, walkers, n_jobs), dim3(MG_WALK_BLOCK), 0,
                       stream, d_jobs, d_frozen, r, lanes, max_rounds);
    return hipGetLastError();
}

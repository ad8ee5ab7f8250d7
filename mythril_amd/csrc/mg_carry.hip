// mg_carry_batch — the two kernels around the interpreter's eval-mode launch
// (host side: mg_carry.h, mg_carry_batch in mg_api.cpp).
//
// mg_carry_fill_kernel, grid (lane tiles, leaves, jobs): blockIdx.z selects a
// device-resident mg_carry_dev_job, blockIdx.y a leaf (leaves beyond the
// grid's y are strided), a thread one lane.  It writes the leaf's eight limb
// rows of the job's leaf region [leaf][limb][lanes]: the pin row broadcast
// where the job's mask pins the leaf, else generator v9 at candidate index
// first_index + lane (mg_carry_gen of mg_carry.h, the function
// mg_carry_fill_host runs).  Consecutive threads take consecutive lanes, so
// each limb row is written coalesced; the job record, the mask word, the pin
// row and the leaf's generator are block-uniform (scalar loads).
//
// mg_carry_gather_kernel, one block per job: the interpreter's first_sat of
// the job (atomicMin over its lanes, lane 0 at candidate index 0) is the first
// lane on which every root holds; that lane's column of the leaf region goes
// to the job's output rows, zero where there is none and past n_leaves.
//
// Neither kernel is compute-bound: a job of 256 lanes and 20 leaves is 160 KB
// written and 640 B gathered.  What the call buys is the fixed launch count.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_carry.h"

__global__ __launch_bounds__(MG_CARRY_TILE) void mg_carry_fill_kernel(
    const mg_carry_dev_job* __restrict__ jobs, uint64_t seed, uint64_t first_index,
    uint32_t lanes) {
    const mg_carry_dev_job* J = jobs + blockIdx.z;                         // block-uniform
    const uint32_t n_leaves = J->n_leaves;
    const uint32_t lane = blockIdx.x * MG_CARRY_TILE + threadIdx.x;
    if (lane >= lanes) return;
    const uint32_t* __restrict__ mask = J->mask;
    const uint32_t* __restrict__ rows = J->rows;
    const mg_leafgen* __restrict__ gen = J->gen;
    const uint32_t* __restrict__ consts = J->consts;
    uint32_t* __restrict__ leaves = J->leaves;
    const uint64_t prog_seed = J->prog_seed;
    for (uint32_t leaf = blockIdx.y; leaf < n_leaves; leaf += gridDim.y)
        mg_carry_fill_lane(mask, rows, gen, consts, prog_seed, seed, first_index, leaf, lane,
                           lanes, lane, leaves);
}

__global__ __launch_bounds__(MG_CARRY_TILE) void mg_carry_gather_kernel(
    const mg_carry_dev_job* __restrict__ jobs, const unsigned long long* __restrict__ first_sat,
    uint32_t lanes, uint32_t max_leaves, long long* __restrict__ out_first,
    uint32_t* __restrict__ out_leaves) {
    const uint32_t g = blockIdx.x;
    const mg_carry_dev_job* J = jobs + g;
    const unsigned long long f = first_sat[g];
    const bool hit = f < lanes;
    const uint32_t n_words = J->n_leaves * 8u, row_words = max_leaves * 8u;
    const uint32_t* __restrict__ leaves = J->leaves;
    uint32_t* __restrict__ out = out_leaves + (uint64_t)g * row_words;
    if (threadIdx.x == 0) out_first[g] = hit ? (long long)f : -1ll;
    for (uint32_t i = threadIdx.x; i < row_words; i += MG_CARRY_TILE)
        out[i] = hit && i < n_words ? leaves[(uint64_t)i * lanes + f] : 0u;
}

// d_jobs: n_jobs records in device memory, every job's leaf region of
// n_leaves x 8 rows of `lanes` words; most_leaves: the largest n_leaves.
hipError_t mg_launch_carry_fill(const mg_carry_dev_job* d_jobs, uint32_t n_jobs,
                                uint32_t most_leaves, uint64_t seed, uint64_t first_index,
                                uint32_t lanes, hipStream_t stream) {
    if (!mg_carry_shared_ok(n_jobs, lanes)) return hipErrorInvalidValue;
    if (most_leaves == 0) return hipSuccess;
    const uint32_t gy = most_leaves < MG_CARRY_GRID_LEAVES ? most_leaves : MG_CARRY_GRID_LEAVES;
    const dim3 grid((lanes + MG_CARRY_TILE - 1) / MG_CARRY_TILE, gy, n_jobs);
    hipLaunchKernelGGL(mg_carry_fill_kernel, grid, dim3(MG_CARRY_TILE), 0, stream, d_jobs, seed,
                       first_index, lanes);
    return hipGetLastError();
}

// d_first: the interpreter's first_sat per job; d_out_first [n_jobs],
// d_out_leaves [n_jobs][max_leaves][8], max_leaves >= every job's n_leaves.
hipError_t mg_launch_carry_gather(const mg_carry_dev_job* d_jobs, uint32_t n_jobs,
                                  const unsigned long long* d_first, uint32_t lanes,
                                  uint32_t max_leaves, long long* d_out_first,
                                  uint32_t* d_out_leaves, hipStream_t stream) {
    if (!mg_carry_shared_ok(n_jobs, lanes)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mg_carry_gather_kernel, dim3(n_jobs), dim3(MG_CARRY_TILE), 0, stream,
                       d_jobs, d_first, lanes, max_leaves, d_out_first, d_out_leaves);
    return hipGetLastError();
}

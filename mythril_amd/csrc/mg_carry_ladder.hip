// mg_carry_ladder — the two kernels around the interpreter's eval-mode launch
// when a job carries a ladder of pin masks (host side:
// mg_carry.h, mg_carry_ladder in mg_api.cpp).
//
// mg_carry_fill_rungs_kernel, grid (column tiles, leaves, jobs): blockIdx.z
// selects a device-resident mg_carry_dev_job, blockIdx.y a leaf (leaves beyond
// the grid's y are strided), a thread one of the job's C = R x lanes columns
// (R: the batch's largest n_rungs).  Column c lies on rung
// min(c / lanes, n_rungs - 1) and holds candidate c % lanes: the pin row where
// that rung's mask pins the leaf, else generator v9 at candidate index
// first_index + c % lanes (mg_carry_fill_rung_lane of mg_carry.h, the function
// mg_carry_fill_rungs_host runs), so every rung replays one candidate stream.
// Consecutive threads take consecutive columns, so each limb row is written
// coalesced; the job record, the pin row and the leaf's generator are
// block-uniform (scalar loads).  The mask word is block-uniform whenever a
// tile lies inside one rung, which is always the case when lanes % 256 == 0
// (and for every tile past a job's last rung boundary); the kernel tests that
// per block and then reads the word through a block-uniform pointer.  A tile
// that straddles a boundary reads it per thread: at most two words per leaf,
// one cache line.
//
// mg_carry_gather_rungs_kernel, one block per job: the interpreter's first_sat
// of the job (atomicMin over its columns, column 0 at candidate index 0) is the
// lowest column on which every root holds, hence a column of the strictest
// rung that has one; that column's rung and its column of the leaf region go
// to the job's outputs, -1 and zero rows where there is none.
//
// Neither kernel is compute-bound: 3 rungs of 256 lanes and 20 leaves are
// 480 KB written and 640 B gathered.  What the ladder buys is that further pin
// sets cost columns of the same three launches, not launches.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_carry.h"

__global__ __launch_bounds__(MG_CARRY_TILE) void mg_carry_fill_rungs_kernel(
    const mg_carry_dev_job* __restrict__ jobs, uint64_t seed, uint64_t first_index,
    uint32_t lanes, uint32_t cols) {
    const mg_carry_dev_job* J = jobs + blockIdx.z;                         // block-uniform
    const uint32_t n_leaves = J->n_leaves, n_rungs = J->n_rungs;
    const uint32_t tile0 = blockIdx.x * MG_CARRY_TILE;
    const uint32_t col = tile0 + threadIdx.x;
    if (col >= cols) return;
    const uint32_t* __restrict__ masks = J->mask;
    const uint32_t* __restrict__ rows = J->rows;
    const mg_leafgen* __restrict__ gen = J->gen;
    const uint32_t* __restrict__ consts = J->consts;
    uint32_t* __restrict__ leaves = J->leaves;
    const uint64_t prog_seed = J->prog_seed;
    const uint32_t words = (n_leaves + 31) / 32;
    const uint32_t tile1 = (cols - tile0 < MG_CARRY_TILE ? cols : tile0 + MG_CARRY_TILE) - 1;
    const uint32_t r0 = mg_carry_rung(tile0, lanes, n_rungs);
    if (r0 == mg_carry_rung(tile1, lanes, n_rungs)) {
        // the whole tile on rung r0: what mg_carry_fill_rung_lane does, with
        // the rung's mask behind a block-uniform pointer
        const uint32_t* __restrict__ mask = masks + (uint64_t)r0 * words;
        const uint32_t lane = col % lanes;
        for (uint32_t leaf = blockIdx.y; leaf < n_leaves; leaf += gridDim.y)
            mg_carry_fill_lane(mask, rows, gen, consts, prog_seed, seed, first_index, leaf, lane,
                               cols, col, leaves);
    } else {
        for (uint32_t leaf = blockIdx.y; leaf < n_leaves; leaf += gridDim.y)
            mg_carry_fill_rung_lane(masks, words, n_rungs, rows, gen, consts, prog_seed, seed,
                                    first_index, leaf, col, lanes, cols, col, leaves);
    }
}

__global__ __launch_bounds__(MG_CARRY_TILE) void mg_carry_gather_rungs_kernel(
    const mg_carry_dev_job* __restrict__ jobs, const unsigned long long* __restrict__ first_sat,
    uint32_t lanes, uint32_t cols, uint32_t max_leaves, long long* __restrict__ out_first,
    long long* __restrict__ out_rung, uint32_t* __restrict__ out_leaves) {
    const uint32_t g = blockIdx.x;
    const mg_carry_dev_job* J = jobs + g;
    const unsigned long long f = first_sat[g];
    const bool hit = f < cols;
    const uint32_t n_words = J->n_leaves * 8u, row_words = max_leaves * 8u;
    const uint32_t* __restrict__ leaves = J->leaves;
    uint32_t* __restrict__ out = out_leaves + (uint64_t)g * row_words;
    if (threadIdx.x == 0) {
        out_first[g] = hit ? (long long)f : -1ll;
        out_rung[g] = hit ? (long long)mg_carry_rung((uint32_t)f, lanes, J->n_rungs) : -1ll;
    }
    for (uint32_t i = threadIdx.x; i < row_words; i += MG_CARRY_TILE)
        out[i] = hit && i < n_words ? leaves[(uint64_t)i * cols + f] : 0u;
}

// d_jobs: n_jobs records in device memory, n_rungs in 1..MG_CARRY_MAX_RUNGS
// each, every job's leaf region of n_leaves x 8 rows of `cols` words; cols: the
// largest n_rungs x lanes; most_leaves: the largest n_leaves.
hipError_t mg_launch_carry_fill_rungs(const mg_carry_dev_job* d_jobs, uint32_t n_jobs,
                                      uint32_t most_leaves, uint64_t seed, uint64_t first_index,
                                      uint32_t lanes, uint32_t cols, hipStream_t stream) {
    if (!mg_carry_shared_ok(n_jobs, lanes) || cols < lanes || cols > MG_REPAIR_MAX_LANES)
        return hipErrorInvalidValue;
    if (most_leaves == 0) return hipSuccess;
    const uint32_t gy = most_leaves < MG_CARRY_GRID_LEAVES ? most_leaves : MG_CARRY_GRID_LEAVES;
    const dim3 grid((cols + MG_CARRY_TILE - 1) / MG_CARRY_TILE, gy, n_jobs);
    hipLaunchKernelGGL(mg_carry_fill_rungs_kernel, grid, dim3(MG_CARRY_TILE), 0, stream, d_jobs,
                       seed, first_index, lanes, cols);
    return hipGetLastError();
}

// d_first: the interpreter's first_sat per job; d_out_first, d_out_rung
// [n_jobs], d_out_leaves [n_jobs][max_leaves][8], max_leaves >= every job's
// n_leaves.
hipError_t mg_launch_carry_gather_rungs(const mg_carry_dev_job* d_jobs, uint32_t n_jobs,
                                        const unsigned long long* d_first, uint32_t lanes,
                                        uint32_t cols, uint32_t max_leaves,
                                        long long* d_out_first, long long* d_out_rung,
                                        uint32_t* d_out_leaves, hipStream_t stream) {
    if (!mg_carry_shared_ok(n_jobs, lanes) || cols < lanes || cols > MG_REPAIR_MAX_LANES)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mg_carry_gather_rungs_kernel, dim3(n_jobs), dim3(MG_CARRY_TILE), 0, stream,
                       d_jobs, d_first, lanes, cols, max_leaves, d_out_first, d_out_rung,
                       d_out_leaves);
    return hipGetLastError();
}

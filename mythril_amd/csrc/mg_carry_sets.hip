// mg_carry_ladder_sets — the fill kernel of a pin ladder whose rungs carry
// their own pin rows (host side: mg_carry.h,
// mg_carry_ladder_sets in mg_api.cpp).  The interpreter's eval-mode launch and
// the gather (mg_carry_gather_rungs_kernel of mg_carry_ladder.hip) follow it
// unchanged: they read leaf regions and know nothing of where a pin came from.
//
// mg_carry_fill_sets_kernel, grid (column tiles, leaves, jobs): blockIdx.z
// selects a device-resident mg_carry_dev_job and the mg_carry_sets_dev_job of
// the same index, blockIdx.y a leaf (leaves beyond the grid's y are strided),
// a thread one of the job's C = R x lanes columns (R: the batch's largest
// n_rungs).  Column c lies on rung r = min(c / lanes, n_rungs - 1) and holds
// candidate c % lanes: where mask r pins the leaf, its row of row set
// rung_set[r], else generator v9 at candidate index first_index + c % lanes
// (mg_carry_fill_set_lane of mg_carry.h, the function mg_carry_fill_sets_host
// runs).  Consecutive threads take consecutive columns, so each limb row is
// written coalesced.  The job records and the leaf's generator are
// block-uniform; the mask word, rung_set[r] and with it the pin row are
// block-uniform whenever a tile lies inside one rung, which is always the case
// when lanes % 256 == 0 (and for every tile past a job's last rung boundary):
// the kernel tests that per block and then reads mask and rows through
// block-uniform pointers (scalar loads).  A tile that straddles a boundary
// reads them per thread: at most two masks and two row sets per leaf.
//
// The kernel is a store stream, not compute-bound, and independent of the
// interpreter's register layout: further witnesses cost columns of the same
// three launches, and no further compile of the group.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_carry.h"

__global__ __launch_bounds__(MG_CARRY_TILE) void mg_carry_fill_sets_kernel(
    const mg_carry_dev_job* __restrict__ jobs, const mg_carry_sets_dev_job* __restrict__ sjobs,
    uint64_t seed, uint64_t first_index, uint32_t lanes, uint32_t cols) {
    const mg_carry_dev_job* J = jobs + blockIdx.z;                         // block-uniform
    const uint32_t n_leaves = J->n_leaves, n_rungs = J->n_rungs;
    const uint32_t tile0 = blockIdx.x * MG_CARRY_TILE;
    const uint32_t col = tile0 + threadIdx.x;
    if (col >= cols) return;
    const uint32_t* __restrict__ masks = J->mask;
    const uint32_t* __restrict__ rows = J->rows;
    const uint32_t* __restrict__ rung_set = sjobs[blockIdx.z].rung_set;
    const mg_leafgen* __restrict__ gen = J->gen;
    const uint32_t* __restrict__ consts = J->consts;
    uint32_t* __restrict__ leaves = J->leaves;
    const uint64_t prog_seed = J->prog_seed;
    const uint32_t words = (n_leaves + 31) / 32;
    const uint32_t tile1 = (cols - tile0 < MG_CARRY_TILE ? cols : tile0 + MG_CARRY_TILE) - 1;
    const uint32_t r0 = mg_carry_rung(tile0, lanes, n_rungs);
    if (r0 == mg_carry_rung(tile1, lanes, n_rungs)) {
        // the whole tile on rung r0: what mg_carry_fill_set_lane does, with the
        // rung's mask and row set behind block-uniform pointers
        const uint32_t* __restrict__ mask = masks + (uint64_t)r0 * words;
        const uint32_t* __restrict__ set = rows + (uint64_t)rung_set[r0] * n_leaves * 8;
        const uint32_t lane = col % lanes;
        for (uint32_t leaf = blockIdx.y; leaf < n_leaves; leaf += gridDim.y)
            mg_carry_fill_lane(mask, set, gen, consts, prog_seed, seed, first_index, leaf, lane,
                               cols, col, leaves);
    } else {
        for (uint32_t leaf = blockIdx.y; leaf < n_leaves; leaf += gridDim.y)
            mg_carry_fill_set_lane(masks, words, n_rungs, rung_set, rows, n_leaves, gen, consts,
                                   prog_seed, seed, first_index, leaf, col, lanes, cols, col,
                                   leaves);
    }
}

// d_jobs, d_sjobs: n_jobs records each in device memory, n_rungs in
// 1..MG_CARRY_MAX_RUNGS, every rung_set entry below the job's n_sets, every
// job's leaf region of n_leaves x 8 rows of `cols` words; cols: the largest
// n_rungs x lanes; most_leaves: the largest n_leaves.
hipError_t mg_launch_carry_fill_sets(const mg_carry_dev_job* d_jobs,
                                     const mg_carry_sets_dev_job* d_sjobs, uint32_t n_jobs,
                                     uint32_t most_leaves, uint64_t seed, uint64_t first_index,
                                     uint32_t lanes, uint32_t cols, hipStream_t stream) {
    if (!mg_carry_shared_ok(n_jobs, lanes) || cols < lanes || cols > MG_REPAIR_MAX_LANES)
        return hipErrorInvalidValue;
    if (most_leaves == 0) return hipSuccess;
    const uint32_t gy = most_leaves < MG_CARRY_GRID_LEAVES ? most_leaves : MG_CARRY_GRID_LEAVES;
    const dim3 grid((cols + MG_CARRY_TILE - 1) / MG_CARRY_TILE, gy, n_jobs);
    hipLaunchKernelGGL(mg_carry_fill_sets_kernel, grid, dim3(MG_CARRY_TILE), 0, stream, d_jobs,
                       d_sjobs, seed, first_index, lanes, cols);
    return hipGetLastError();
}

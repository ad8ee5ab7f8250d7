// mg_census_batch — the verdict censuses of several programs over one chunk of
// candidates in one launch (host side: mg_census_batch.h,
// mg_census_batch in mg_api.cpp).
//
// Grid (blocks, jobs).  blockIdx.y selects a device-resident
// mg_census_batch_job: the rows of the job's first mask probe in its probe
// region, its root count and its counter block.  The work is the single
// census's own (mg_census_block of mg_census_block.h, which mg_census_kernel
// calls too), so job g's counters are those of mg_census_kernel on it alone:
// sums and minima only, whatever the number of blocks that share its tiles.
// The row stride, the candidate count, the first index and the offset are the
// same for all jobs and arrive as launch arguments.
//
// The job record is read block-uniformly (scalar loads), and its pointers
// reach the body as __restrict__ parameters: read through the record inside
// the loops, the compiler has to assume that the counter atomics alias them
// and reloads them (DESIGN.md §3.16 measured that on the walk's kernels).
// LDS is the body's static 24.6 KB, as in the single kernel.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_census_batch.h"
#include "mg_census_block.h"

static_assert(MG_CENSUS_BATCH_TILE == MG_CENSUS_BLOCK, "the blocks rule counts the body's tiles");

__global__ __launch_bounds__(MG_CENSUS_BLOCK) void mg_census_batch_kernel(
    const mg_census_batch_job* __restrict__ jobs, uint64_t stride, uint64_t n, uint64_t first,
    uint64_t offset) {
    const mg_census_batch_job* J = jobs + blockIdx.y;                      // block-uniform
    mg_census_block(J->rows, stride, n, J->n_roots, first, offset, J->out);
}

// d_jobs: n_jobs records in device memory.  Every job's rows hold `stride`
// words each, n <= stride of them written; offset + n stays below 2^53.
hipError_t mg_launch_census_batch(const mg_census_batch_job* d_jobs, uint32_t n_jobs,
                                  uint64_t stride, uint64_t n, uint64_t first, uint64_t offset,
                                  hipStream_t stream) {
    if (n == 0 || n_jobs == 0) return hipSuccess;
    if (n_jobs > MG_CENSUS_BATCH_MAX_JOBS || n > stride ||
        offset + n > (1ull << MG_CENSUS_OFFSET_BITS))
        return hipErrorInvalidValue;
    const uint32_t blocks = mg_census_batch_blocks(n_jobs, n);
    hipLaunchKernelGGL(mg_census_batch_kernel, dim3(blocks, n_jobs), dim3(MG_CENSUS_BLOCK), 0,
                       stream, d_jobs, stride, n, first, offset);
    return hipGetLastError();
}

// mg_census — per-constraint verdict census of a chunk of candidates
// (specification: mythril_amd/census.py reduce_masks).
//
// One launch per chunk: the block body is mg_census_block (mg_census_block.h,
// which says what it reduces and how), shared with the batched census
// (mg_census_batch.hip).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_census.h"
#include "mg_census_block.h"

#define BLOCK MG_CENSUS_BLOCK
// blocks per launch: 8 per CU of a 256-CU part; tiles beyond are grid-strided
#define MAX_BLOCKS 2048u

__global__ __launch_bounds__(BLOCK) void mg_census_kernel(
    const uint32_t* __restrict__ rows, uint64_t stride, uint64_t n, uint32_t n_roots,
    uint64_t first, uint64_t offset, unsigned long long* __restrict__ out) {
    mg_census_block(rows, stride, n, n_roots, first, offset, out);
}

hipError_t mg_launch_census(const uint32_t* d_rows, uint64_t stride, uint64_t n, uint32_t n_roots,
                            uint64_t first, uint64_t offset, unsigned long long* d_out,
                            hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n_roots == 0 || n_roots > MG_CENSUS_MAX_ROOTS || n > stride ||
        offset + n > (1ull << MG_CENSUS_OFFSET_BITS))
        return hipErrorInvalidValue;
    const uint64_t tiles = (n + BLOCK - 1) / BLOCK;
    const uint32_t blocks = tiles < MAX_BLOCKS ? (uint32_t)tiles : MAX_BLOCKS;
    hipLaunchKernelGGL(mg_census_kernel, dim3(blocks), dim3(BLOCK), 0, stream, d_rows, stride, n,
                       n_roots, first, offset, d_out);
    return hipGetLastError();
}

/* The block body of the verdict census: what one
 * 256-thread block of mg_census_kernel (mg_census.hip) does, and of
 * mg_census_batch_kernel (mg_census_batch.hip) for the job its blockIdx.y
 * names.  Device code; specification: mythril_amd/census.py reduce_masks.
 *
 * The interpreter wrote, for every lane of the chunk, the verdict mask of the
 * program's constraints as probe values: bit k of the mask = constraint
 * ("root") k holds.  Probe p carries roots 256p .. 256p + 255, so root k is
 * bit k % 32 of row k / 32 of the probe buffer ([probe][limb][lane] u32, one
 * row per limb).  One lane = one candidate: it reads the ceil(n_roots / 32)
 * rows that hold roots (coalesced dwords, one pass) and the block reduces
 *   pass[k]        candidates on which root k holds       (ballot + popcount)
 *   first_block[k] candidates whose lowest failing root is k
 *   sole_block[k]  candidates whose only failing root is k
 *   sole_index[k]  the smallest such candidate index
 *   nfail_hist[f]  candidates with exactly f failing roots
 *   best           min over candidates of (failing roots, candidate index)
 * into LDS counters, flushed with one 64-bit atomic per non-zero counter.
 * Sums and minima only: the result does not depend on the order of blocks,
 * launches or chunk sizes, nor on how many blocks share the tiles. */
#ifndef MG_CENSUS_BLOCK_H
#define MG_CENSUS_BLOCK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_census.h"

#define MG_CENSUS_BLOCK 256

/* Tiles of 256 candidates are strided over gridDim.x from blockIdx.x; the
 * other grid dimensions are the caller's.  rows: the first row of the first
 * mask probe, `stride` words per row; out: the counter block mg_census.h lays
 * out for n_roots. */
static __device__ __forceinline__ void mg_census_block(
    const uint32_t* __restrict__ rows, uint64_t stride, uint64_t n, uint32_t n_roots,
    uint64_t first, uint64_t offset, unsigned long long* __restrict__ out) {
    __shared__ uint32_t s_pass[MG_CENSUS_MAX_ROOTS];
    __shared__ uint32_t s_first[MG_CENSUS_MAX_ROOTS];
    __shared__ uint32_t s_sole[MG_CENSUS_MAX_ROOTS];
    __shared__ uint32_t s_hist[MG_CENSUS_MAX_ROOTS + 1];
    __shared__ unsigned long long s_sole_index[MG_CENSUS_MAX_ROOTS];
    __shared__ unsigned long long s_best;

    const uint32_t tid = threadIdx.x;
    const uint32_t l = tid & 63;
    for (uint32_t k = tid; k < n_roots; k += MG_CENSUS_BLOCK) {
        s_pass[k] = 0;
        s_first[k] = 0;
        s_sole[k] = 0;
        s_hist[k] = 0;
        s_sole_index[k] = ~0ull;
    }
    if (tid == 0) {
        s_hist[n_roots] = 0;
        s_best = ~0ull;
    }
    __syncthreads();

    const uint32_t n_words = (n_roots + 31) / 32;
    const uint64_t tiles = (n + MG_CENSUS_BLOCK - 1) / MG_CENSUS_BLOCK;
    unsigned long long best = ~0ull;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // uniform per block
        const uint64_t gid = tile * MG_CENSUS_BLOCK + tid;
        const bool active = gid < n;        // lanes past n: the interpreter wrote nothing
        uint32_t nfail = 0, first_fail = 0;
        for (uint32_t q = 0; q < n_words; ++q) {
            const uint32_t bits = n_roots - 32 * q < 32 ? n_roots - 32 * q : 32;
            const uint32_t valid = bits == 32 ? ~0u : (1u << bits) - 1u;   // bits >= n_roots: ignored
            const uint32_t word = active ? rows[(uint64_t)q * stride + gid] & valid : 0u;
            const uint32_t fail = active ? ~word & valid : 0u;
            if (fail && !nfail) first_fail = 32 * q + __builtin_ctz(fail);
            nfail += __builtin_popcount(fail);
            // lane b of the wave keeps the wave's count of root 32q + b
            uint32_t cnt = 0;
            for (uint32_t b = 0; b < bits; ++b) {
                const unsigned long long m = __ballot((word >> b) & 1u);
                if (l == b) cnt = (uint32_t)__builtin_popcountll(m);
            }
            if (cnt) atomicAdd(&s_pass[32 * q + l], cnt);
        }
        if (active) {
            atomicAdd(&s_hist[nfail], 1u);
            if (nfail) atomicAdd(&s_first[first_fail], 1u);
            if (nfail == 1) {
                atomicAdd(&s_sole[first_fail], 1u);
                atomicMin(&s_sole_index[first_fail], (unsigned long long)(first + gid));
            }
            const unsigned long long key =
                ((unsigned long long)nfail << MG_CENSUS_OFFSET_BITS) | (offset + gid);
            best = key < best ? key : best;
        }
    }
    if (best != ~0ull) atomicMin(&s_best, best);
    __syncthreads();

    unsigned long long* g_pass = out + mg_census_pass(n_roots);
    unsigned long long* g_first = out + mg_census_first(n_roots);
    unsigned long long* g_sole = out + mg_census_sole(n_roots);
    unsigned long long* g_hist = out + mg_census_hist(n_roots);
    unsigned long long* g_sole_index = out + mg_census_sole_index(n_roots);
    for (uint32_t k = tid; k <= n_roots; k += MG_CENSUS_BLOCK) {
        if (s_hist[k]) atomicAdd(g_hist + k, (unsigned long long)s_hist[k]);
        if (k == n_roots) break;
        if (s_pass[k]) atomicAdd(g_pass + k, (unsigned long long)s_pass[k]);
        if (s_first[k]) atomicAdd(g_first + k, (unsigned long long)s_first[k]);
        if (s_sole[k]) {
            atomicAdd(g_sole + k, (unsigned long long)s_sole[k]);
            atomicMin(g_sole_index + k, s_sole_index[k]);
        }
    }
    if (tid == 0 && s_best != ~0ull) atomicMin(out + mg_census_best(n_roots), s_best);
}

#endif

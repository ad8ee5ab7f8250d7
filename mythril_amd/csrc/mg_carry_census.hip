// mg_carry_census — the two kernels after the interpreter's eval-mode launch
// when a pin ladder is censused instead of gathered (host
// side: mg_carry.h, mg_carry_census in mg_api.cpp).  The fill kernel is
// mg_carry_fill_rungs_kernel of mg_carry_ladder.hip, unchanged.
//
// mg_carry_census_kernel, grid (tiles, rungs, jobs): block (., r, j) returns at
// once when job j has no rung r; else it is one block of the verdict census
// (mg_census_block of mg_census_block.h, the body mg_census_kernel and
// mg_census_batch_kernel run) on the L = lanes columns r x L .. r x L + L - 1
// of the job's mask rows, rows of C = cols words, into counter block (j, r).
// first = offset = r x L, so sole_index and best come out as column numbers.
// The surplus columns of a job with fewer rungs than the batch are evaluated
// by the interpreter and read by nobody.
//
// mg_carry_starts_kernel, one block per job: the start rule of mg_carry.h
// (mg_carry_pick_starts is its sequential form) and the gather of the W start
// columns' leaf rows.  The bests are ranked by the first n_rungs threads.  The
// sole part of the list, up to 8 x 1024 entries in (rung, root) order, is
// compacted 256 entries a pass: every thread tests one entry
// (mg_carry_sole_entry), a wave ballot and the popcount of the lanes below give
// the place inside the wave, the four waves' totals go through LDS and are
// prefixed by every thread, and the loop ends as soon as W starts are known —
// with the bests in front that is before the first pass when W <= n_rungs.
// The counters are read only: both kernels' global writes are the census
// body's atomics and plain vector stores.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_carry.h"
#include "mg_census_batch.h"
#include "mg_census_block.h"

static_assert(MG_CARRY_TILE == MG_CENSUS_BLOCK, "both kernels run the census body's block");

__global__ __launch_bounds__(MG_CENSUS_BLOCK) void mg_carry_census_kernel(
    const mg_carry_dev_job* __restrict__ jobs, const mg_carry_census_dev_job* __restrict__ cjobs,
    uint32_t lanes, uint32_t cols) {
    const uint32_t r = blockIdx.y;
    if (r >= jobs[blockIdx.z].n_rungs) return;                             // block-uniform
    const mg_carry_census_dev_job* K = cjobs + blockIdx.z;
    const uint32_t n_roots = K->n_roots;
    const uint64_t col0 = (uint64_t)r * lanes;
    mg_census_block(K->mrows + col0, cols, lanes, n_roots, col0, col0,
                    K->counts + (uint64_t)r * mg_census_words(n_roots));
}

__global__ __launch_bounds__(MG_CARRY_TILE) void mg_carry_starts_kernel(
    const mg_carry_dev_job* __restrict__ jobs, const mg_carry_census_dev_job* __restrict__ cjobs,
    uint32_t walkers, uint32_t cols, uint32_t max_leaves, long long* __restrict__ out_col,
    uint32_t* __restrict__ out_nfail, uint32_t* __restrict__ out_rows) {
    __shared__ long long s_col[MG_CARRY_MAX_WALKERS];
    __shared__ uint32_t s_nfail[MG_CARRY_MAX_WALKERS];
    __shared__ uint32_t s_wave[MG_CARRY_TILE / 64];
    __shared__ uint32_t s_best;

    const uint32_t g = blockIdx.x, tid = threadIdx.x, l = tid & 63, wave = tid >> 6;
    const mg_carry_dev_job* J = jobs + g;                                  // block-uniform
    const mg_carry_census_dev_job* K = cjobs + g;
    const unsigned long long* __restrict__ counts = K->counts;
    const uint32_t n_roots = K->n_roots, n_rungs = J->n_rungs;

    // the bests, by (failing roots, rung): wave 0, one rung per lane
    if (wave == 0) {
        unsigned long long b = ~0ull;
        uint32_t rank = n_rungs;
        if (tid < n_rungs) {
            b = mg_carry_rung_best(counts, n_roots, tid);
            rank = mg_carry_best_rank(counts, n_roots, n_rungs, tid);
        }
        if (rank < n_rungs && rank < walkers) {
            s_col[rank] = (long long)(b & MG_CARRY_COL_MASK);
            s_nfail[rank] = (uint32_t)(b >> MG_CENSUS_OFFSET_BITS);
        }
        const unsigned long long m = __ballot(rank < n_rungs);
        if (tid == 0) s_best = (uint32_t)__builtin_popcountll(m);
    }
    __syncthreads();

    // the sole columns in (rung, root) order, 256 entries a pass
    uint32_t n = s_best;                                                   // uniform
    const uint32_t entries = n_rungs * n_roots;
    for (uint32_t e0 = 0; e0 < entries && n < walkers; e0 += MG_CARRY_TILE) {
        const uint32_t e = e0 + tid;
        unsigned long long col = 0;
        const bool take = e < entries && mg_carry_sole_entry(counts, n_roots, e, &col);
        const unsigned long long m = __ballot(take);
        const uint32_t below = (uint32_t)__builtin_popcountll(m & ((1ull << l) - 1ull));
        if (l == 0) s_wave[wave] = (uint32_t)__builtin_popcountll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < MG_CARRY_TILE / 64; ++w) {
            const uint32_t c = s_wave[w];
            before += w < wave ? c : 0u;
            total += c;
        }
        const uint32_t at = n + before + below;
        if (take && at < walkers) {
            s_col[at] = (long long)col;
            s_nfail[at] = 1u;
        }
        __syncthreads();
        n += total;
    }
    if (n > walkers) n = walkers;

    // start w: list[w], past the end list[0]; -1 when the job counted nothing
    const uint32_t n_words = J->n_leaves * 8u, row_words = max_leaves * 8u;
    const uint32_t* __restrict__ leaves = J->leaves;
    if (tid < walkers) {
        const uint32_t src = tid < n ? tid : 0u;
        out_col[(uint64_t)g * walkers + tid] = n ? s_col[src] : -1ll;
        out_nfail[(uint64_t)g * walkers + tid] = n ? s_nfail[src] : 0xFFFFFFFFu;
    }
    for (uint32_t w = 0; w < walkers; ++w) {
        const long long c = n ? s_col[w < n ? w : 0u] : -1ll;
        const bool ok = c >= 0 && c < (long long)cols;
        uint32_t* __restrict__ out = out_rows + ((uint64_t)g * walkers + w) * row_words;
        for (uint32_t i = tid; i < row_words; i += MG_CARRY_TILE)
            out[i] = ok && i < n_words ? leaves[(uint64_t)i * cols + (uint64_t)c] : 0u;
    }
}

// d_jobs, d_cjobs: n_jobs records each in device memory; every job's mask rows
// hold `cols` words each, cols = rungs x lanes with rungs the largest n_rungs;
// every counter block preset (sums zero, minima all ones).
hipError_t mg_launch_carry_census(const mg_carry_dev_job* d_jobs,
                                  const mg_carry_census_dev_job* d_cjobs, uint32_t n_jobs,
                                  uint32_t rungs, uint32_t lanes, uint32_t cols,
                                  hipStream_t stream) {
    if (!mg_carry_shared_ok(n_jobs, lanes) || rungs < 1 || rungs > MG_CARRY_MAX_RUNGS ||
        (uint64_t)rungs * lanes != cols || cols > MG_REPAIR_MAX_LANES)
        return hipErrorInvalidValue;
    const uint32_t tiles = mg_census_batch_blocks(n_jobs * rungs, lanes);
    hipLaunchKernelGGL(mg_carry_census_kernel, dim3(tiles, rungs, n_jobs), dim3(MG_CENSUS_BLOCK),
                       0, stream, d_jobs, d_cjobs, lanes, cols);
    return hipGetLastError();
}

// d_out_col, d_out_nfail [n_jobs][walkers], d_out_rows
// [n_jobs][walkers][max_leaves][8], max_leaves >= every job's n_leaves.
hipError_t mg_launch_carry_starts(const mg_carry_dev_job* d_jobs,
                                  const mg_carry_census_dev_job* d_cjobs, uint32_t n_jobs,
                                  uint32_t walkers, uint32_t cols, uint32_t max_leaves,
                                  long long* d_out_col, uint32_t* d_out_nfail,
                                  uint32_t* d_out_rows, hipStream_t stream) {
    if (n_jobs < 1 || n_jobs > MG_CARRY_MAX_JOBS || walkers < 1 ||
        walkers > MG_CARRY_MAX_WALKERS || cols < 1 || cols > MG_REPAIR_MAX_LANES ||
        max_leaves > MG_CARRY_MAX_LEAVES)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mg_carry_starts_kernel, dim3(n_jobs), dim3(MG_CARRY_TILE), 0, stream, d_jobs,
                       d_cjobs, walkers, cols, max_leaves, d_out_col, d_out_nfail, d_out_rows);
    return hipGetLastError();
}

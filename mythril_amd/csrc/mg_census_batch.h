/* mg_census_batch: the censuses of several programs over one
 * candidate range in one launch sequence.  Host part, plain C++ with no HIP
 * call: the shape of a job, the checks of its counts, the chunk rule, the
 * blocks rule and the plan of the batch's device buffer; the ABI
 * (mg_census_batch, mg_census_batch_plan_host, mg_census_batch_blocks_host)
 * and the CPU suite run this code.  The job record is laid out as the kernel
 * of mg_census_batch.hip reads it.
 *
 * One device buffer holds the whole batch, every region 256-byte aligned, in
 * this order:
 *   descs                     one mg_pdesc per job (a program in several jobs
 *                             is copied per job): the interpreter's table
 *   jobs                      one mg_census_batch_job per job
 *   per job, its counters     the block mg_census.h lays out for the job's own
 *                             n_roots, at a common stride: mg_census_words of
 *                             the largest n_roots, rounded up to 256 bytes
 *     (up to here one upload from a host image of the same layout: the sums
 *      zero, the minima all ones; the counters come back in one copy)
 *   per job, its probe region max n_probes x 8 x lanes words, the maximum over
 *                             the batch, rounded up to 256 bytes: the stride
 *                             the interpreter's shell applies
 * lanes: the candidates of the largest launch, min(n_cand, chunk).
 * offsets[]: MG_CB_SHARED shared regions, then MG_CB_JOB_REGIONS per job. */
#ifndef MG_CENSUS_BATCH_H
#define MG_CENSUS_BATCH_H

#include <stdint.h>
#include <stdio.h>
#include "mythgpu.h"
#include "mythgpu_ir.h"
#include "mg_device.h"
#include "mg_census.h"

enum { MG_CB_DESCS, MG_CB_JOBS, MG_CB_SHARED };
enum { MG_CB_COUNTS, MG_CB_PROBES, MG_CB_JOB_REGIONS };
#define MG_CB_OFF(g, k) ((size_t)MG_CB_SHARED + (size_t)(g) * MG_CB_JOB_REGIONS + (k))

static_assert(MG_CENSUS_BATCH_SHARED == MG_CB_SHARED &&
              MG_CENSUS_BATCH_JOB_REGIONS == MG_CB_JOB_REGIONS,
              "include/mythgpu.h documents the length of the offset table");

/* blocks of one launch over all jobs: the single kernel's MAX_BLOCKS */
#define MG_CENSUS_BATCH_GRID 2048u
#define MG_CENSUS_BATCH_TILE 256u

/* The job as the kernel reads it: blockIdx.y selects one. */
struct mg_census_batch_job {
    const uint32_t* rows;       /* in its probe region: row 0 of its first mask probe */
    unsigned long long* out;    /* its counter block */
    uint32_t n_roots;
    uint32_t pad;
};

/* why a plan is refused (mg_census_batch_why words them) */
enum {
    MG_CB_OK, MG_CB_NULL, MG_CB_N_JOBS, MG_CB_CHUNK_MULTIPLE, MG_CB_CHUNK_BYTES, MG_CB_NO_FIT,
    MG_CB_OVERFLOW
};

static inline bool mg_census_roots_ok(uint32_t n_roots) {
    return n_roots >= 1 && n_roots <= MG_CENSUS_MAX_ROOTS;
}

/* the mask probes of n_roots roots from mask_probe0 on are probes of the program */
static inline bool mg_census_mask_ok(uint32_t n_probes, uint32_t n_roots, uint32_t mask_probe0) {
    const uint32_t n_mask = n_roots / 256u + (n_roots % 256u ? 1u : 0u);
    return mask_probe0 < n_probes && n_mask <= n_probes - mask_probe0;
}

/* What mg_census accepts for the counts of one job. */
static inline bool mg_census_shape_ok(const mg_census_shape& s) {
    return mg_census_roots_ok(s.n_roots) && mg_census_mask_ok(s.n_probes, s.n_roots, s.mask_probe0);
}

/* Blocks per job of one launch over n candidates: the whole grid stays near
 * MG_CENSUS_BATCH_GRID, a job has at least one block and no more than tiles. */
static inline uint32_t mg_census_batch_blocks(uint32_t n_jobs, uint64_t n) {
    if (n_jobs == 0 || n == 0) return 0;
    const uint64_t tiles = n / MG_CENSUS_BATCH_TILE + (n % MG_CENSUS_BATCH_TILE ? 1 : 0);
    uint32_t per = MG_CENSUS_BATCH_GRID / n_jobs;
    if (per < 1) per = 1;
    return tiles < per ? (uint32_t)tiles : per;
}

/* a + round_up(count * unit, 256) into *a; false when 64 bits overflow */
static inline bool mg_cb_add(uint64_t* a, uint64_t count, uint64_t unit) {
    uint64_t b;
    if (__builtin_mul_overflow(count, unit, &b)) return false;
    if (__builtin_add_overflow(b, (uint64_t)255, &b)) return false;
    b &= ~(uint64_t)255;
    return !__builtin_add_overflow(*a, b, a);
}

/* Every offset of the batch's buffer, its size and the chunk.  The shapes need
 * not have passed mg_census_shape_ok: sizes are computed with checked
 * arithmetic.  chunk 0: the largest multiple of 256, at most MG_CENSUS_CHUNK,
 * at which the probe regions of all jobs fit MG_CENSUS_MAX_PROBE_BYTES; an
 * explicit chunk is taken or refused.  Returns MG_CB_OK or the reason;
 * *need: with MG_CB_CHUNK_BYTES the bytes the probe regions would take, with
 * MG_CB_NO_FIT those at 256 lanes.  *count_stride_w (u64 words) and
 * *probe_stride_w (u32 words): the distance between two jobs' regions (may be
 * NULL). */
static inline int mg_census_batch_plan(const mg_census_shape* shapes, uint32_t n_jobs,
                                       uint64_t n_cand, uint64_t chunk, uint64_t* offsets,
                                       uint64_t* bytes, uint64_t* out_chunk, uint64_t* need,
                                       uint64_t* count_stride_w, uint64_t* probe_stride_w) {
    if (!shapes || !offsets || !bytes || !out_chunk || !need) return MG_CB_NULL;
    *need = 0;
    if (n_jobs < 1 || n_jobs > MG_CENSUS_BATCH_MAX_JOBS) return MG_CB_N_JOBS;
    if (chunk % MG_CENSUS_BATCH_TILE) return MG_CB_CHUNK_MULTIPLE;
    uint32_t max_probes = 0, max_roots = 0;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        max_probes = shapes[g].n_probes > max_probes ? shapes[g].n_probes : max_probes;
        max_roots = shapes[g].n_roots > max_roots ? shapes[g].n_roots : max_roots;
    }
    /* bytes of all probe regions per lane: below 2^45 */
    const uint64_t lane_b = (uint64_t)max_probes * 32u * n_jobs;
    if (chunk) {
        if (__builtin_mul_overflow(lane_b, chunk, need)) return MG_CB_OVERFLOW;
        if (*need > MG_CENSUS_MAX_PROBE_BYTES) return MG_CB_CHUNK_BYTES;
    } else {
        chunk = MG_CENSUS_CHUNK;
        if (lane_b && chunk > MG_CENSUS_MAX_PROBE_BYTES / lane_b)
            chunk = MG_CENSUS_MAX_PROBE_BYTES / lane_b / MG_CENSUS_BATCH_TILE * MG_CENSUS_BATCH_TILE;
        if (chunk == 0) {
            *need = lane_b * MG_CENSUS_BATCH_TILE;
            return MG_CB_NO_FIT;
        }
    }
    *out_chunk = chunk;
    const uint64_t lanes = n_cand < chunk ? n_cand : chunk;
    uint64_t at = 0;
    offsets[MG_CB_DESCS] = at;
    if (!mg_cb_add(&at, n_jobs, sizeof(mg_pdesc))) return MG_CB_OVERFLOW;
    offsets[MG_CB_JOBS] = at;
    if (!mg_cb_add(&at, n_jobs, sizeof(mg_census_batch_job))) return MG_CB_OVERFLOW;
    /* 5 r + 2 words of 8 bytes, r below 2^32 */
    uint64_t count_b = 0, probe_b = 0;
    if (!mg_cb_add(&count_b, 5 * (uint64_t)max_roots + 2, 8)) return MG_CB_OVERFLOW;
    if (!mg_cb_add(&probe_b, (uint64_t)max_probes * 32u, lanes)) return MG_CB_OVERFLOW;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        offsets[MG_CB_OFF(g, MG_CB_COUNTS)] = at;
        if (__builtin_add_overflow(at, count_b, &at)) return MG_CB_OVERFLOW;
    }
    for (uint32_t g = 0; g < n_jobs; ++g) {
        offsets[MG_CB_OFF(g, MG_CB_PROBES)] = at;
        if (__builtin_add_overflow(at, probe_b, &at)) return MG_CB_OVERFLOW;
    }
    *bytes = at;
    if (count_stride_w) *count_stride_w = count_b / 8;
    if (probe_stride_w) *probe_stride_w = probe_b / 4;
    return MG_CB_OK;
}

/* The refusal in words (what follows "census_batch: " in the ABI's message). */
static inline void mg_census_batch_why(int status, uint32_t n_jobs, uint64_t chunk, uint64_t need,
                                       char* buf, size_t len) {
    if (!buf || !len) return;
    switch (status) {
    case MG_CB_OK: buf[0] = 0; break;
    case MG_CB_NULL: snprintf(buf, len, "null argument"); break;
    case MG_CB_N_JOBS:
        snprintf(buf, len, "%u jobs outside 1..%u", n_jobs, MG_CENSUS_BATCH_MAX_JOBS);
        break;
    case MG_CB_CHUNK_MULTIPLE:
        snprintf(buf, len, "chunk %llu is not a multiple of %u", (unsigned long long)chunk,
                 MG_CENSUS_BATCH_TILE);
        break;
    case MG_CB_CHUNK_BYTES:
        snprintf(buf, len, "%llu bytes needed for the probe regions of %u jobs at chunk %llu, "
                 "at most %llu; pass a smaller chunk or 0",
                 (unsigned long long)need, n_jobs, (unsigned long long)chunk,
                 (unsigned long long)MG_CENSUS_MAX_PROBE_BYTES);
        break;
    case MG_CB_NO_FIT:
        snprintf(buf, len, "%llu bytes needed for the probe regions of %u jobs at %u candidates "
                 "per chunk exceed a %llu MiB probe buffer; load the census view of the programs "
                 "(census.census_view: only the mask probes are written) or pass fewer jobs",
                 (unsigned long long)need, n_jobs, MG_CENSUS_BATCH_TILE,
                 (unsigned long long)(MG_CENSUS_MAX_PROBE_BYTES >> 20));
        break;
    default: snprintf(buf, len, "the batch's buffer exceeds 64 bits"); break;
    }
}

#endif

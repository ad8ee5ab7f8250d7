/* mg_carry_batch: remembered witnesses evaluated on the
 * programs of the groups that extend them, many jobs in one launch sequence.
 * Host part, plain C++ with no HIP call: the candidate generator v9 restated
 * for host and device (include/mythgpu.h states it above mg_leafgen,
 * oracle/gen_ref.py is its specification), the lane function of the fill
 * kernel, the checks of a batch's counts and the plan of its device buffer;
 * the ABI (mg_carry_batch, mg_carry_fill_host, mg_carry_plan_host), the kernels
 * of mg_carry.hip and the CPU suite run this code.
 *
 * Lane i of a job evaluates the candidate whose pinned leaves (bit l of the
 * job's mask) are the job's pin rows and whose free leaves are the generator's
 * values at candidate index first_index + i, each masked to the leaf's width.
 *
 * One device buffer holds the whole batch, every region 256-byte aligned, in
 * this order:
 *   descs                one mg_pdesc per job: the interpreter's table
 *   jobs                 one mg_carry_dev_job per job
 *   first                one u64 per job, preset all ones: the interpreter's
 *                        first_sat (lane 0 has candidate index 0 there)
 *   per job              its pin mask, its pin rows, its leaf generators
 *     (up to here one upload from a host image of the same layout)
 *   out                  n_jobs i64 (first, -1: none), then n_jobs x
 *                        max_leaves x 8 words: one download
 *   per job, its leaves  [leaf][limb][lanes] at a common stride: the largest
 *                        n_leaves of the batch x 8 x lanes words, rounded up to
 *                        256 bytes (the stride the interpreter's shell applies)
 * offsets[]: MG_CY_SHARED shared regions, then MG_CY_JOB_REGIONS per job.
 *
 * mg_carry_ladder runs the same sequence with n_rungs pin
 * masks per job, strictest first: with R the batch's largest n_rungs a job has
 * C = R x lanes columns, column c on rung min(c / lanes, n_rungs - 1) and
 * candidate c % lanes (mg_carry_rung, mg_carry_fill_rung_lane).  Its buffer is
 * the one above with a job's mask region holding its n_rungs masks one after
 * the other, the output block n_jobs i64 first, n_jobs i64 rung and the rows,
 * and leaf regions of C columns (mg_carry_ladder_plan).
 *
 * mg_carry_ladder_sets is the ladder with n_sets row sets
 * per job: rung r pins from row set rung_set[r] (mg_carry_fill_set_lane).  Its
 * buffer is the ladder's with a job's rows region holding its n_sets row sets
 * one after the other, and before the output block one record per job and
 * every job's rung_set (mg_carry_sets_plan, after the ladder's plan).
 *
 * mg_carry_census adds per-rung counter blocks, probe
 * regions and an output block of W starts to the ladder's buffer
 * (mg_carry_census_plan, at the end of this file, with the start rule). */
#ifndef MG_CARRY_H
#define MG_CARRY_H

#include <stdint.h>
#include "mythgpu.h"
#include "mythgpu_ir.h"
#include "mg_device.h"
#include "mg_repair.h"
#include "mg_census.h"

enum { MG_CY_DESCS, MG_CY_JOBS, MG_CY_FIRST, MG_CY_OUT, MG_CY_SHARED };
enum { MG_CY_MASK, MG_CY_ROWS, MG_CY_GEN, MG_CY_LEAVES, MG_CY_JOB_REGIONS };
#define MG_CY_OFF(g, k) ((size_t)MG_CY_SHARED + (size_t)(g) * MG_CY_JOB_REGIONS + (k))

static_assert(MG_CARRY_SHARED == MG_CY_SHARED && MG_CARRY_JOB_REGIONS == MG_CY_JOB_REGIONS,
              "include/mythgpu.h documents the length of the offset table");

#define MG_CARRY_TILE 256u
/* leaves of one fill launch along the grid's y; leaves beyond are strided */
#define MG_CARRY_GRID_LEAVES 1024u

#define MG_CARRY_FN MG_REPAIR_FN

/* The job as the kernels read it: blockIdx.z (fill) / blockIdx.x (gather). */
struct mg_carry_dev_job {
    const uint32_t* mask;       /* [(n_leaves + 31) / 32] */
    const uint32_t* rows;       /* [n_leaves][8] */
    const mg_leafgen* gen;      /* [n_leaves], as loaded */
    const uint32_t* consts;     /* the program's constant table */
    uint32_t* leaves;           /* its leaf region [n_leaves][8][lanes] */
    uint64_t prog_seed;
    uint32_t n_leaves;
    uint32_t n_rungs;           /* mg_carry_ladder: the masks at `mask`; else 0 */
};

#define MG_CARRY_GOLD 0x9E3779B97F4A7C15ull
#define MG_CARRY_MIX1 0xBF58476D1CE4E5B9ull
#define MG_CARRY_SALT_P 0xD1B54A32D192ED03ull
#define MG_CARRY_SALT_L 0x8CB92BA72F3D8DD7ull
#define MG_CARRY_CLS_MUL 0x2545F491u

MG_CARRY_FN uint64_t mg_carry_salt(uint64_t prog_seed, uint32_t leaf) {
    return (prog_seed * MG_CARRY_SALT_P) ^ (((uint64_t)leaf + 1) * MG_CARRY_SALT_L);
}

/* the class of leaf `leaf` for the 64 candidates around idx: 0 .. 99 */
MG_CARRY_FN uint32_t mg_carry_class(uint64_t seed, uint64_t prog_seed, uint32_t leaf,
                                    uint64_t idx) {
    const uint64_t ss = seed ^ mg_carry_salt(prog_seed, leaf);
    const uint32_t y = (((uint32_t)(idx >> 6) ^ (uint32_t)ss) * MG_CARRY_CLS_MUL) ^
                       (uint32_t)(ss >> 32);
    return mg_repair_mulhi(y, 100u);
}

/* which branch a class takes: 0 r0 (64 bits), 1 boundary, 2 pool, 3 uniform */
MG_CARRY_FN uint32_t mg_carry_branch(const mg_leafgen& g, uint32_t cls) {
    if (g.pct_uniform <= cls && cls < g.pct_small) return 0;
    if (g.pct_small <= cls && cls < g.pct_boundary) return 1;
    if (cls >= g.pct_boundary && g.pool_n > 0) return 2;
    return 3;
}

/* Generator v9: the value of leaf `leaf` at candidate index idx, masked to the
 * leaf's width, upper limbs zero.  consts: the program's constant table (read
 * at pool_off .. pool_off + pool_n - 1 in the pool class only). */
MG_CARRY_FN void mg_carry_gen(uint64_t seed, uint64_t prog_seed, uint32_t leaf, uint64_t idx,
                              const mg_leafgen& g, const uint32_t* consts, uint32_t* v) {
    uint64_t s = (seed ^ mg_carry_salt(prog_seed, leaf) ^ idx) + MG_CARRY_GOLD;
    const uint64_t u = s ^ (s >> 32);
    const uint64_t z = u * MG_CARRY_MIX1;
    const uint64_t r0 = z ^ (z >> 32);
    const uint32_t lo = (uint32_t)r0;
    const uint32_t w = g.width;
    const uint32_t br = mg_carry_branch(g, mg_carry_class(seed, prog_seed, leaf, idx));
    for (uint32_t k = 0; k < 8; ++k) v[k] = 0;
    if (br == 0) {
        v[0] = lo;
        v[1] = (uint32_t)(r0 >> 32);
    } else if (br == 1) {
        const uint32_t kind = mg_repair_mulhi(lo, 6u);
        const uint32_t k = mg_repair_mulhi(lo * 0x9E3779B1u, w);
        if (kind == 1) {
            v[0] = 1;
        } else if (kind == 2) {
            mg_repair_addpow(v, w - 1, false);
        } else if (kind == 3) {
            for (uint32_t i = 0; i < 8; ++i) v[i] = 0xFFFFFFFFu;
        } else if (kind == 4) {
            mg_repair_addpow(v, k, false);
            mg_repair_addpow(v, 0, false);
        } else if (kind == 5) {
            mg_repair_addpow(v, k, false);
            mg_repair_addpow(v, 0, true);
        }
    } else if (br == 2) {
        const uint32_t e = g.pool_off + mg_repair_mulhi(lo, g.pool_n);
        const uint32_t delta = mg_repair_mulhi(lo * 0x85EBCA6Bu, 3u);
        for (uint32_t k = 0; k < 8; ++k) v[k] = consts[(uint64_t)e * 8 + k];
        if (delta != 1) mg_repair_addpow(v, 0, delta == 0);
    } else {
        const uint32_t x = lo ^ (uint32_t)(r0 >> 32);
        const uint32_t c[3] = {0x85EBCA6Bu, 0xC2B2AE35u, 0x27D4EB2Fu};
        v[0] = lo;
        v[1] = (uint32_t)(r0 >> 32);
        for (uint32_t k = 0; k < 3; ++k) {
            const uint64_t p = (uint64_t)x * c[k] + r0;
            v[2 * k + 2] = (uint32_t)p;
            v[2 * k + 3] = (uint32_t)(p >> 32);
        }
    }
    mg_repair_mask(v, w);
}

MG_CARRY_FN bool mg_carry_pinned(const uint32_t* mask, uint32_t leaf) {
    return (mask[leaf >> 5] >> (leaf & 31)) & 1u;
}

/* The fill kernel's lane function: leaf `leaf` of lane `lane` of a job into
 * column `col` of rows of `stride` words: out[(leaf * 8 + k) * stride + col]. */
MG_CARRY_FN void mg_carry_fill_lane(const uint32_t* mask, const uint32_t* rows,
                                    const mg_leafgen* gen, const uint32_t* consts,
                                    uint64_t prog_seed, uint64_t seed, uint64_t first_index,
                                    uint32_t leaf, uint32_t lane, uint64_t stride, uint64_t col,
                                    uint32_t* out) {
    uint32_t v[8];
    if (mg_carry_pinned(mask, leaf)) {
        for (uint32_t k = 0; k < 8; ++k) v[k] = rows[(uint64_t)leaf * 8 + k];
        mg_repair_mask(v, gen[leaf].width);
    } else {
        mg_carry_gen(seed, prog_seed, leaf, first_index + lane, gen[leaf], consts, v);
    }
    for (uint32_t k = 0; k < 8; ++k) out[((uint64_t)leaf * 8 + k) * stride + col] = v[k];
}

/* the rung of column col of a job of n_rungs masks at `lanes` candidates per
 * rung: a job with fewer rungs than the batch repeats its last one */
MG_CARRY_FN uint32_t mg_carry_rung(uint32_t col, uint32_t lanes, uint32_t n_rungs) {
    const uint32_t r = col / lanes;
    return r < n_rungs ? r : n_rungs - 1;
}

/* The rung fill kernel's lane function: leaf `leaf` of column `col` of a job
 * whose n_rungs masks of `words` words each lie one after the other at
 * `masks`: mg_carry_fill_lane under the mask of the column's rung, at
 * candidate col % lanes, into out[(leaf * 8 + k) * stride + out_col]. */
MG_CARRY_FN void mg_carry_fill_rung_lane(const uint32_t* masks, uint32_t words, uint32_t n_rungs,
                                         const uint32_t* rows, const mg_leafgen* gen,
                                         const uint32_t* consts, uint64_t prog_seed,
                                         uint64_t seed, uint64_t first_index, uint32_t leaf,
                                         uint32_t col, uint32_t lanes, uint64_t stride,
                                         uint64_t out_col, uint32_t* out) {
    const uint32_t r = mg_carry_rung(col, lanes, n_rungs);
    mg_carry_fill_lane(masks + (uint64_t)r * words, rows, gen, consts, prog_seed, seed,
                       first_index, leaf, col % lanes, stride, out_col, out);
}

/* The set fill kernel's lane function: mg_carry_fill_rung_lane for a job whose
 * n_sets row sets of n_leaves x 8 words each lie one after the other at
 * `rows`; the column's rung r pins from row set rung_set[r]. */
MG_CARRY_FN void mg_carry_fill_set_lane(const uint32_t* masks, uint32_t words, uint32_t n_rungs,
                                        const uint32_t* rung_set, const uint32_t* rows,
                                        uint32_t n_leaves, const mg_leafgen* gen,
                                        const uint32_t* consts, uint64_t prog_seed, uint64_t seed,
                                        uint64_t first_index, uint32_t leaf, uint32_t col,
                                        uint32_t lanes, uint64_t stride, uint64_t out_col,
                                        uint32_t* out) {
    const uint32_t r = mg_carry_rung(col, lanes, n_rungs);
    mg_carry_fill_lane(masks + (uint64_t)r * words, rows + (uint64_t)rung_set[r] * n_leaves * 8,
                       gen, consts, prog_seed, seed, first_index, leaf, col % lanes, stride,
                       out_col, out);
}

/* the shared counts mg_carry_batch accepts */
static inline bool mg_carry_shared_ok(uint32_t n_jobs, uint32_t lanes) {
    return n_jobs >= 1 && n_jobs <= MG_CARRY_MAX_JOBS && lanes >= 1 &&
           lanes <= MG_REPAIR_MAX_LANES;
}

/* what the generator reads of a leaf table is inside the constants */
static inline bool mg_carry_gen_ok(const mg_leafgen* gen, uint32_t n_leaves, uint32_t n_consts) {
    for (uint32_t l = 0; l < n_leaves; ++l) {
        if (gen[l].width < 1 || gen[l].width > 256) return false;
        if (gen[l].pool_n && (gen[l].pool_off > n_consts || gen[l].pool_n > n_consts - gen[l].pool_off))
            return false;
    }
    return true;
}

/* a + round_up(count * unit, 256) into *a; false when 64 bits overflow */
static inline bool mg_cy_add(uint64_t* a, uint64_t count, uint64_t unit) {
    uint64_t b;
    if (__builtin_mul_overflow(count, unit, &b)) return false;
    if (__builtin_add_overflow(b, (uint64_t)255, &b)) return false;
    b &= ~(uint64_t)255;
    return !__builtin_add_overflow(*a, b, a);
}

/* The uploaded front of every carry buffer: descriptors, job records, first
 * words, then job by job its masks (n_rungs[g] of them, NULL: one each), row
 * sets (n_sets[g] of them, NULL: one each) and generators.  *at: where the
 * front ends; *most: the largest n_leaves. */
static inline bool mg_cy_plan_front(const uint32_t* n_leaves, const uint32_t* n_rungs,
                                    const uint32_t* n_sets, uint32_t n_jobs, uint64_t* offsets,
                                    uint64_t* at_out, uint32_t* most_out) {
    uint64_t at = 0;
    offsets[MG_CY_DESCS] = at;
    if (!mg_cy_add(&at, n_jobs, sizeof(mg_pdesc))) return false;
    offsets[MG_CY_JOBS] = at;
    if (!mg_cy_add(&at, n_jobs, sizeof(mg_carry_dev_job))) return false;
    offsets[MG_CY_FIRST] = at;
    if (!mg_cy_add(&at, n_jobs, 8)) return false;
    uint32_t most = 0;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const uint64_t n = n_leaves[g];
        most = n_leaves[g] > most ? n_leaves[g] : most;
        offsets[MG_CY_OFF(g, MG_CY_MASK)] = at;
        if (!mg_cy_add(&at, (n + 31) / 32 * (n_rungs ? n_rungs[g] : 1u), 4)) return false;
        offsets[MG_CY_OFF(g, MG_CY_ROWS)] = at;
        if (!mg_cy_add(&at, n * (n_sets ? n_sets[g] : 1u), 32)) return false;
        offsets[MG_CY_OFF(g, MG_CY_GEN)] = at;
        if (!mg_cy_add(&at, n, sizeof(mg_leafgen))) return false;
    }
    *at_out = at;
    *most_out = most;
    return true;
}

/* The downloaded block and the leaf regions from *at on: out_job bytes of
 * output per job, then every job's leaf region of most x 8 x cols words,
 * rounded up to 256 bytes. */
static inline bool mg_cy_plan_back(uint32_t n_jobs, uint32_t most, uint64_t cols, uint64_t out_job,
                                   uint64_t* offsets, uint64_t* at_io, uint64_t* leaf_stride_w) {
    uint64_t at = *at_io;
    offsets[MG_CY_OUT] = at;
    uint64_t out_b;
    if (__builtin_mul_overflow(out_job, (uint64_t)n_jobs, &out_b)) return false;
    if (!mg_cy_add(&at, out_b, 1)) return false;
    uint64_t leaf_b = 0;
    if (!mg_cy_add(&leaf_b, (uint64_t)most * 32u, cols)) return false;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        offsets[MG_CY_OFF(g, MG_CY_LEAVES)] = at;
        if (__builtin_add_overflow(at, leaf_b, &at)) return false;
    }
    *at_io = at;
    if (leaf_stride_w) *leaf_stride_w = leaf_b / 4;
    return true;
}

/* The layout mg_carry_batch and mg_carry_ladder share: job g has n_rungs[g]
 * masks (NULL: one each), the output block out_fixed bytes per job before its
 * rows, a leaf region `cols` columns. */
static inline bool mg_cy_plan(const uint32_t* n_leaves, const uint32_t* n_rungs, uint32_t n_jobs,
                              uint64_t cols, uint32_t out_fixed, uint32_t max_leaves,
                              uint64_t* offsets, uint64_t* bytes, uint64_t* leaf_stride_w) {
    uint64_t at = 0;
    uint32_t most = 0;
    if (!mg_cy_plan_front(n_leaves, n_rungs, nullptr, n_jobs, offsets, &at, &most)) return false;
    if (!mg_cy_plan_back(n_jobs, most, cols, (uint64_t)max_leaves * 32u + out_fixed, offsets, &at,
                         leaf_stride_w))
        return false;
    *bytes = at;
    return true;
}

/* Every offset of the batch's buffer and its size; false when the shared
 * counts are out of range or 64 bits overflow.  n_leaves[g] need not be below
 * max_leaves: sizes are computed with checked arithmetic.  *leaf_stride_w (u32
 * words, may be NULL): the distance between two jobs' leaf regions. */
static inline bool mg_carry_plan(const uint32_t* n_leaves, uint32_t n_jobs, uint32_t lanes,
                                 uint32_t max_leaves, uint64_t* offsets, uint64_t* bytes,
                                 uint64_t* leaf_stride_w) {
    if (!n_leaves || !offsets || !bytes || !mg_carry_shared_ok(n_jobs, lanes)) return false;
    return mg_cy_plan(n_leaves, nullptr, n_jobs, lanes, 8, max_leaves, offsets, bytes,
                      leaf_stride_w);
}

/* the shared counts mg_carry_ladder accepts; *cols (may be NULL): the columns
 * of a job, the batch's largest n_rungs x lanes */
static inline bool mg_carry_ladder_ok(const uint32_t* n_rungs, uint32_t n_jobs, uint32_t lanes,
                                      uint32_t* cols) {
    if (!n_rungs || !mg_carry_shared_ok(n_jobs, lanes)) return false;
    uint32_t most = 0;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        if (n_rungs[g] < 1 || n_rungs[g] > MG_CARRY_MAX_RUNGS) return false;
        most = n_rungs[g] > most ? n_rungs[g] : most;
    }
    if ((uint64_t)most * lanes > MG_REPAIR_MAX_LANES) return false;
    if (cols) *cols = most * lanes;
    return true;
}

/* mg_carry_plan for mg_carry_ladder: masks of n_rungs[g] x words, an output
 * block of first, rung and rows, leaf regions of the batch's largest n_leaves
 * x 8 x C words. */
static inline bool mg_carry_ladder_plan(const uint32_t* n_leaves, const uint32_t* n_rungs,
                                        uint32_t n_jobs, uint32_t lanes, uint32_t max_leaves,
                                        uint64_t* offsets, uint64_t* bytes,
                                        uint64_t* leaf_stride_w) {
    uint32_t cols = 0;
    if (!n_leaves || !offsets || !bytes || !mg_carry_ladder_ok(n_rungs, n_jobs, lanes, &cols))
        return false;
    return mg_cy_plan(n_leaves, n_rungs, n_jobs, cols, 16, max_leaves, offsets, bytes,
                      leaf_stride_w);
}

/* mg_carry_ladder_sets: the ladder's buffer with n_sets[g]
 * row sets in job g's rows region and two kinds of region more, in this order:
 *   descs, jobs, first, per job masks, row sets, generators  as the ladder
 *   set records           one mg_carry_sets_dev_job per job
 *   per job, its rung_set n_rungs u32: the row set of every rung
 *     (up to here one upload)
 *   out, per job its leaves                                  as the ladder
 * offsets[]: the ladder's table, then MG_CS_SHARED entries, then
 * MG_CS_JOB_REGIONS per job. */
enum { MG_CS_RECORDS, MG_CS_SHARED };
enum { MG_CS_RUNG_SET, MG_CS_JOB_REGIONS };
#define MG_CS_BASE(n_jobs) ((size_t)MG_CY_SHARED + (size_t)(n_jobs) * MG_CY_JOB_REGIONS)
#define MG_CS_OFF(n_jobs, g, k) \
    (MG_CS_BASE(n_jobs) + MG_CS_SHARED + (size_t)(g) * MG_CS_JOB_REGIONS + (k))
#define MG_CS_TABLE(n_jobs) (MG_CS_BASE(n_jobs) + MG_CS_SHARED + (size_t)(n_jobs) * MG_CS_JOB_REGIONS)

static_assert(MG_CARRY_SETS_SHARED == MG_CS_SHARED &&
              MG_CARRY_SETS_JOB_REGIONS == MG_CS_JOB_REGIONS,
              "include/mythgpu.h documents the length of the offset table");

/* What the set fill kernel reads of a job beside its mg_carry_dev_job (same
 * index), whose `rows` is the first of the job's n_sets row sets. */
struct mg_carry_sets_dev_job {
    const uint32_t* rung_set;   /* [n_rungs], each below n_sets */
    uint32_t n_sets;
    uint32_t pad;
};

/* every rung of a job names one of its row sets */
static inline bool mg_carry_rung_set_ok(const uint32_t* rung_set, uint32_t n_rungs,
                                        uint32_t n_sets) {
    if (!rung_set) return false;
    for (uint32_t r = 0; r < n_rungs; ++r)
        if (rung_set[r] >= n_sets) return false;
    return true;
}

/* the shared counts mg_carry_ladder_sets accepts: the ladder's, and 1 to
 * MG_CARRY_MAX_SETS row sets per job */
static inline bool mg_carry_sets_ok(const uint32_t* n_rungs, const uint32_t* n_sets,
                                    uint32_t n_jobs, uint32_t lanes, uint32_t* cols) {
    if (!n_sets || !mg_carry_ladder_ok(n_rungs, n_jobs, lanes, cols)) return false;
    for (uint32_t g = 0; g < n_jobs; ++g)
        if (n_sets[g] < 1 || n_sets[g] > MG_CARRY_MAX_SETS) return false;
    return true;
}

/* mg_carry_ladder_plan for mg_carry_ladder_sets. */
static inline bool mg_carry_sets_plan(const uint32_t* n_leaves, const uint32_t* n_rungs,
                                      const uint32_t* n_sets, uint32_t n_jobs, uint32_t lanes,
                                      uint32_t max_leaves, uint64_t* offsets, uint64_t* bytes,
                                      uint64_t* leaf_stride_w) {
    uint32_t cols = 0;
    if (!n_leaves || !offsets || !bytes || !mg_carry_sets_ok(n_rungs, n_sets, n_jobs, lanes, &cols))
        return false;
    uint64_t at = 0;
    uint32_t most = 0;
    if (!mg_cy_plan_front(n_leaves, n_rungs, n_sets, n_jobs, offsets, &at, &most)) return false;
    offsets[MG_CS_BASE(n_jobs) + MG_CS_RECORDS] = at;
    if (!mg_cy_add(&at, n_jobs, sizeof(mg_carry_sets_dev_job))) return false;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        offsets[MG_CS_OFF(n_jobs, g, MG_CS_RUNG_SET)] = at;
        if (!mg_cy_add(&at, n_rungs[g], 4)) return false;
    }
    if (!mg_cy_plan_back(n_jobs, most, cols, (uint64_t)max_leaves * 32u + 16u, offsets, &at,
                         leaf_stride_w))
        return false;
    *bytes = at;
    return true;
}

/* mg_carry_census: the ladder's fill and evaluation, then a
 * verdict census of every rung's own columns and W start columns per job.
 * Its buffer is the ladder's with three kinds of region more, in this order:
 *   descs, jobs, first, per job masks, rows, generators      as the ladder
 *   census records        one mg_carry_census_dev_job per job
 *   per job, its counters n_rungs blocks of mg_census_words(n_roots) u64 one
 *                         after the other, as mg_census.h lays a block out
 *     (up to here one upload: the sums zero, the minima all ones)
 *   out                   start_col [n_jobs][W] i64, start_nfail [n_jobs][W]
 *                         u32, starts [n_jobs][W][max_leaves][8] u32
 *     (counters and out come back in one download)
 *   per job, its leaves   as the ladder, C columns
 *   per job, its probes   [probe][limb][C] at a common stride: the largest
 *                         n_probes of the batch x 8 x C words, rounded up to
 *                         256 bytes (the stride the interpreter's shell applies)
 * offsets[]: the ladder's table, then MG_CC_SHARED entries, then
 * MG_CC_JOB_REGIONS per job. */
enum { MG_CC_RECORDS, MG_CC_SHARED };
enum { MG_CC_COUNTS, MG_CC_PROBES, MG_CC_JOB_REGIONS };
#define MG_CC_BASE(n_jobs) ((size_t)MG_CY_SHARED + (size_t)(n_jobs) * MG_CY_JOB_REGIONS)
#define MG_CC_OFF(n_jobs, g, k) \
    (MG_CC_BASE(n_jobs) + MG_CC_SHARED + (size_t)(g) * MG_CC_JOB_REGIONS + (k))
#define MG_CC_TABLE(n_jobs) (MG_CC_BASE(n_jobs) + MG_CC_SHARED + (size_t)(n_jobs) * MG_CC_JOB_REGIONS)

static_assert(MG_CARRY_CENSUS_SHARED == MG_CC_SHARED &&
              MG_CARRY_CENSUS_JOB_REGIONS == MG_CC_JOB_REGIONS,
              "include/mythgpu.h documents the length of the offset table");

/* What the census and starts kernels read of a job beside its mg_carry_dev_job
 * (same index). */
struct mg_carry_census_dev_job {
    const uint32_t* mrows;      /* in its probe region: row 0 of its first mask probe */
    unsigned long long* counts; /* its n_rungs counter blocks */
    uint32_t n_roots;
    uint32_t pad;
};

/* why a plan is refused (mg_carry_census words them) */
enum {
    MG_CC_OK, MG_CC_NULL, MG_CC_LADDER, MG_CC_WALKERS, MG_CC_ROOTS, MG_CC_MASK, MG_CC_OVERFLOW
};

/* bytes of the output block per job */
static inline uint64_t mg_carry_census_out_job(uint32_t walkers, uint32_t max_leaves) {
    return (uint64_t)walkers * (12u + (uint64_t)max_leaves * 32u);
}

/* Every offset of mg_carry_census's buffer and its size, with checked
 * arithmetic.  *bad (may be NULL): the job a per-job refusal names.
 * *probe_stride_w (u32 words, may be NULL): the distance between two jobs'
 * probe regions. */
static inline int mg_carry_census_plan(const uint32_t* n_leaves, const uint32_t* n_rungs,
                                       const uint32_t* n_roots, const uint32_t* n_probes,
                                       const uint32_t* mask_probe0, uint32_t n_jobs,
                                       uint32_t lanes, uint32_t walkers, uint32_t max_leaves,
                                       uint64_t* offsets, uint64_t* bytes,
                                       uint64_t* leaf_stride_w, uint64_t* probe_stride_w,
                                       uint32_t* bad) {
    if (!n_leaves || !n_roots || !n_probes || !mask_probe0 || !offsets || !bytes)
        return MG_CC_NULL;
    uint32_t cols = 0;
    if (!mg_carry_ladder_ok(n_rungs, n_jobs, lanes, &cols)) return MG_CC_LADDER;
    if (walkers < 1 || walkers > MG_CARRY_MAX_WALKERS) return MG_CC_WALKERS;
    uint32_t most_probes = 0;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        if (bad) *bad = g;
        if (n_roots[g] < 1 || n_roots[g] > MG_CENSUS_MAX_ROOTS) return MG_CC_ROOTS;
        const uint32_t n_mask = (n_roots[g] + 255u) / 256u;
        if (mask_probe0[g] >= n_probes[g] || n_mask > n_probes[g] - mask_probe0[g])
            return MG_CC_MASK;
        most_probes = n_probes[g] > most_probes ? n_probes[g] : most_probes;
    }
    uint64_t at = 0;
    uint32_t most = 0;
    if (!mg_cy_plan_front(n_leaves, n_rungs, nullptr, n_jobs, offsets, &at, &most))
        return MG_CC_OVERFLOW;
    offsets[MG_CC_BASE(n_jobs) + MG_CC_RECORDS] = at;
    if (!mg_cy_add(&at, n_jobs, sizeof(mg_carry_census_dev_job))) return MG_CC_OVERFLOW;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        offsets[MG_CC_OFF(n_jobs, g, MG_CC_COUNTS)] = at;
        if (!mg_cy_add(&at, (uint64_t)mg_census_words(n_roots[g]) * n_rungs[g], 8))
            return MG_CC_OVERFLOW;
    }
    if (!mg_cy_plan_back(n_jobs, most, cols, mg_carry_census_out_job(walkers, max_leaves), offsets,
                         &at, leaf_stride_w))
        return MG_CC_OVERFLOW;
    uint64_t probe_b = 0;
    if (!mg_cy_add(&probe_b, (uint64_t)most_probes * 32u, cols)) return MG_CC_OVERFLOW;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        offsets[MG_CC_OFF(n_jobs, g, MG_CC_PROBES)] = at;
        if (__builtin_add_overflow(at, probe_b, &at)) return MG_CC_OVERFLOW;
    }
    *bytes = at;
    if (probe_stride_w) *probe_stride_w = probe_b / 4;
    return MG_CC_OK;
}

/* The start rule (include/mythgpu.h states it above mg_carry_census;
 * carry.starts_ref is its specification).  counts: a job's n_rungs counter
 * blocks of mg_census_words(n_roots) words one after the other.
 *
 * The list: the bests of the rungs that counted a column, by (failing roots,
 * rung) ascending; then, rung by rung and root by root, every sole_index that
 * is set and is not its rung's best column (1 failing root each).  No column
 * comes twice: rungs own disjoint column ranges, so two entries of different
 * rungs differ; within a rung a column is the sole candidate of at most one
 * root (its only failing root), and a rung's best with one failing root is
 * the lowest column with one failing root, hence the lowest sole column of
 * that root — the one entry the rule leaves out; a best with zero or several
 * failing roots is no sole column at all. */
MG_CARRY_FN unsigned long long mg_carry_rung_best(const unsigned long long* counts,
                                                  uint32_t n_roots, uint32_t r) {
    return counts[(uint64_t)r * mg_census_words(n_roots) + mg_census_best(n_roots)];
}

#define MG_CARRY_COL_MASK ((1ull << MG_CENSUS_OFFSET_BITS) - 1)

/* the per-entry predicate: entry e = r * n_roots + k of the sole part of the
 * list exists; *col: its column */
MG_CARRY_FN bool mg_carry_sole_entry(const unsigned long long* counts, uint32_t n_roots,
                                     uint32_t e, unsigned long long* col) {
    const uint32_t r = e / n_roots, k = e % n_roots;
    const unsigned long long si =
        counts[(uint64_t)r * mg_census_words(n_roots) + mg_census_sole_index(n_roots) + k];
    const unsigned long long best = mg_carry_rung_best(counts, n_roots, r);
    *col = si;
    return si != ~0ull && (best == ~0ull || si != (best & MG_CARRY_COL_MASK));
}

/* the place of rung r's best among the bests, or n_rungs when the rung counted
 * no column */
MG_CARRY_FN uint32_t mg_carry_best_rank(const unsigned long long* counts, uint32_t n_roots,
                                        uint32_t n_rungs, uint32_t r) {
    const unsigned long long mine = mg_carry_rung_best(counts, n_roots, r);
    if (mine == ~0ull) return n_rungs;
    const unsigned long long f = mine >> MG_CENSUS_OFFSET_BITS;
    uint32_t rank = 0;
    for (uint32_t q = 0; q < n_rungs; ++q) {
        const unsigned long long other = mg_carry_rung_best(counts, n_roots, q);
        if (other == ~0ull || q == r) continue;
        const unsigned long long g = other >> MG_CENSUS_OFFSET_BITS;
        if (g < f || (g == f && q < r)) ++rank;
    }
    return rank;
}

/* The rule in sequential form: start_col [walkers] (-1: the job counted no
 * column at all), start_nfail [walkers] (0xFFFFFFFF then). */
static inline void mg_carry_pick_starts(const unsigned long long* counts, uint32_t n_roots,
                                        uint32_t n_rungs, uint32_t walkers, int64_t* start_col,
                                        uint32_t* start_nfail) {
    uint32_t n = 0;
    for (uint32_t place = 0; place < n_rungs && n < walkers; ++place)
        for (uint32_t r = 0; r < n_rungs; ++r)
            if (mg_carry_best_rank(counts, n_roots, n_rungs, r) == place) {
                const unsigned long long b = mg_carry_rung_best(counts, n_roots, r);
                start_col[n] = (int64_t)(b & MG_CARRY_COL_MASK);
                start_nfail[n++] = (uint32_t)(b >> MG_CENSUS_OFFSET_BITS);
                break;
            }
    for (uint32_t e = 0; e < n_rungs * n_roots && n < walkers; ++e) {
        unsigned long long col;
        if (!mg_carry_sole_entry(counts, n_roots, e, &col)) continue;
        start_col[n] = (int64_t)col;
        start_nfail[n++] = 1;
    }
    for (uint32_t w = n; w < walkers; ++w) {
        start_col[w] = n ? start_col[0] : -1;
        start_nfail[w] = n ? start_nfail[0] : 0xFFFFFFFFu;
    }
}

#endif

/* mg_walk_batch: the walks of several groups in one launch
 * sequence.  Host part, plain C++ with no HIP call: the shape of a job, the
 * checks of its counts and the plan of the batch's device buffer; the ABI
 * (mg_walk_batch, mg_walk_batch_plan_host) and the CPU suite run this code.
 * The job is laid out as the kernels of mg_walk_batch.hip read it.
 *
 * One device buffer holds the whole batch, every region 256-byte aligned, in
 * this order:
 *   descs, jobs, frozen       what the interpreter and the kernels read
 *   per job, the tables       bases, gen, roots, atoms, code, entries, pieces,
 *                             fixed, lin, slots, funcs, cands, ukeys
 *     (up to here one upload from a host image of the same layout)
 *   per job, zeroed state     trace, rstate, lives, mstate, ustate, sstate
 *     (one memset)
 *   states, per job dests     all bits set (one memset)
 *   root bits                 [jobs][ceil(walkers * lanes / 64)] u64
 *   per job, its leaf region  max_leaves x 8 x walkers x lanes words, the
 *                             maximum over the batch, rounded up to 256 bytes:
 *                             the stride the interpreter's shell applies
 *   per job, its probe region max_probes x 8 x walkers x lanes words, likewise
 * offsets[]: MG_WB_SHARED shared regions, then MG_WB_JOB_REGIONS per job. */
#ifndef MG_WALK_BATCH_H
#define MG_WALK_BATCH_H

#include <stdint.h>
#include "mythgpu.h"
#include "mythgpu_ir.h"
#include "mg_device.h"
#include "mg_walk_sum.h"
#include "mg_walk_tree.h"

/* shared regions */
enum { MG_WB_DESCS, MG_WB_JOBS, MG_WB_FROZEN, MG_WB_STATES, MG_WB_ROOTBITS, MG_WB_SHARED };
/* regions of one job: uploaded, zeroed, all-ones, scratch */
enum {
    MG_WB_BASES, MG_WB_GEN, MG_WB_ROOTS, MG_WB_ATOMS, MG_WB_CODE, MG_WB_ENTRIES, MG_WB_PIECES,
    MG_WB_FIXED, MG_WB_LIN, MG_WB_SLOTS, MG_WB_FUNCS, MG_WB_CANDS, MG_WB_UKEYS,
    MG_WB_TRACE, MG_WB_RSTATE, MG_WB_LIVES, MG_WB_MSTATE, MG_WB_USTATE, MG_WB_SSTATE,
    MG_WB_DESTS, MG_WB_LEAVES, MG_WB_PROBES, MG_WB_JOB_REGIONS
};
#define MG_WB_FIRST_ZEROED MG_WB_TRACE
#define MG_WB_OFF(g, k) ((size_t)MG_WB_SHARED + (size_t)(g) * MG_WB_JOB_REGIONS + (k))

static_assert(MG_WALK_BATCH_SHARED == MG_WB_SHARED && MG_WALK_BATCH_JOB_REGIONS == MG_WB_JOB_REGIONS,
              "include/mythgpu.h documents the length of the offset table");

/* The job as the kernels read it: device pointers into the batch's buffer
 * (consts: into the loaded program), counts and the seed.  blockIdx.z selects
 * one; whether it is frozen is word blockIdx.z of a separate array, which is
 * also the interpreter's skip_prog, so one copy freezes a job everywhere. */
struct mg_walk_batch_job {
    uint32_t* bases;
    const mg_leafgen* gen;
    const uint32_t* consts;
    const uint32_t *roots, *atoms, *code;
    const uint32_t *entries, *pieces, *fixed, *lin;
    const uint32_t *slots, *funcs, *cands, *ukeys;
    uint32_t *rstate, *mstate, *sstate, *ustate, *dests, *lives;
    mg_walk_state* state;
    uint32_t* trace;
    uint32_t* leaves;           /* the job's leaf region */
    const uint32_t* masks;      /* in its probe region: the root mask rows ... */
    const uint32_t* amasks;
    const uint32_t* resid;
    const uint32_t* srows;
    const uint32_t* urows;
    uint64_t seed;
    uint32_t n_leaves, n_roots, n_atoms, n_resid, n_entries, n_srows, n_urows, n_slots;
};

/* The ranges mg_walk_sum accepts for the counts of one job (what it checks
 * before it looks into a table), so that every size below fits. */
static inline bool mg_walk_batch_shape_ok(const mg_walk_shape& s) {
    if (s.n_leaves == 0 || s.n_probes == 0) return false;
    if (s.n_roots < 1 || s.n_roots > MG_WT_MAX_ROOTS || s.n_atoms > MG_WT_MAX_ATOMS ||
        s.n_code > MG_WT_MAX_CODE)
        return false;
    if (s.n_entries > MG_AIM_MAX_ENTRIES || s.n_srows > MG_SUM_MAX_ROWS ||
        s.n_slots > MG_UF_MAX_SLOTS || s.n_funcs > MG_UF_MAX_FUNCS ||
        s.n_cands > MG_UF_MAX_CANDS || s.n_urows > MG_UF_MAX_ROWS)
        return false;
    /* the root mask, the atom mask, the residuals, the side rows and the U
     * rows are probes of the program, from mask_probe0 on */
    uint64_t need = (uint64_t)s.mask_probe0 + (s.n_roots + 255u) / 256u +
                    (s.n_atoms + 255u) / 256u;
    need += (uint64_t)s.n_resid + s.n_srows + s.n_urows;
    return need <= s.n_probes;
}

static inline bool mg_walk_batch_shared_ok(uint32_t n_jobs, uint32_t walkers, uint32_t lanes,
                                           uint32_t max_rounds) {
    return n_jobs >= 1 && n_jobs <= MG_WALK_BATCH_MAX_JOBS && walkers >= 1 &&
           walkers <= MG_WALK_MAX_WALKERS && lanes >= 1 && lanes <= MG_REPAIR_MAX_LANES &&
           max_rounds >= 1 && max_rounds <= MG_REPAIR_MAX_ROUNDS;
}

/* a + round_up(count * unit, 256) into *a; false when 64 bits overflow */
static inline bool mg_wb_add(uint64_t* a, uint64_t count, uint64_t unit) {
    uint64_t b;
    if (__builtin_mul_overflow(count, unit, &b)) return false;
    if (__builtin_add_overflow(b, (uint64_t)255, &b)) return false;
    b &= ~(uint64_t)255;
    return !__builtin_add_overflow(*a, b, a);
}

/* Every offset of the batch's buffer and its size.  The shapes need not have
 * passed mg_walk_batch_shape_ok: sizes are computed with checked arithmetic,
 * and a total beyond 64 bits is refused.  *leaf_stride_w / *probe_stride_w
 * (may be NULL): the distance between two jobs' regions, in words. */
static inline bool mg_walk_batch_plan(const mg_walk_shape* shapes, uint32_t n_jobs,
                                      uint32_t walkers, uint32_t lanes, uint32_t max_rounds,
                                      uint64_t* offsets, uint64_t* bytes,
                                      uint64_t* leaf_stride_w, uint64_t* probe_stride_w) {
    if (!shapes || !offsets || !bytes) return false;
    if (!mg_walk_batch_shared_ok(n_jobs, walkers, lanes, max_rounds)) return false;
    const uint64_t total = (uint64_t)walkers * lanes, w = walkers;
    uint64_t at = 0;
    offsets[MG_WB_DESCS] = at;
    if (!mg_wb_add(&at, n_jobs, sizeof(mg_pdesc))) return false;
    offsets[MG_WB_JOBS] = at;
    if (!mg_wb_add(&at, n_jobs, sizeof(mg_walk_batch_job))) return false;
    offsets[MG_WB_FROZEN] = at;
    if (!mg_wb_add(&at, n_jobs, 4)) return false;
    uint32_t max_leaves = 0, max_probes = 0;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_walk_shape& s = shapes[g];
        max_leaves = s.n_leaves > max_leaves ? s.n_leaves : max_leaves;
        max_probes = s.n_probes > max_probes ? s.n_probes : max_probes;
        const uint64_t up[MG_WB_FIRST_ZEROED][2] = {
            {w * s.n_leaves, 32}, {s.n_leaves, sizeof(mg_leafgen)}, {s.n_roots, 4},
            {s.n_atoms, 4}, {s.n_code, 4}, {s.n_entries, 20}, {s.n_pieces, 16},
            {s.n_entries, 32}, {s.n_entries, 4}, {s.n_slots, 8}, {s.n_funcs, 12},
            {s.n_cands, 24}, {s.n_ukeys, 32}};
        for (uint32_t k = 0; k < MG_WB_FIRST_ZEROED; ++k) {
            offsets[MG_WB_OFF(g, k)] = at;
            if (!mg_wb_add(&at, up[k][0], up[k][1])) return false;
        }
    }
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_walk_shape& s = shapes[g];
        const uint64_t mwords = (uint64_t)(((uint64_t)s.n_roots + 255u) / 256u) * 8u +
                                (uint64_t)(((uint64_t)s.n_atoms + 255u) / 256u) * 8u;
        const uint64_t zero[MG_WB_DESTS - MG_WB_FIRST_ZEROED][2] = {
            {w * max_rounds, 8}, {w * s.n_resid, 32}, {w * MG_AIM_LIVE_WORDS, 4},
            {w * mwords, 4}, {w * s.n_urows, 32}, {w * s.n_srows, 32}};
        for (uint32_t k = MG_WB_FIRST_ZEROED; k < MG_WB_DESTS; ++k) {
            offsets[MG_WB_OFF(g, k)] = at;
            if (!mg_wb_add(&at, zero[k - MG_WB_FIRST_ZEROED][0], zero[k - MG_WB_FIRST_ZEROED][1]))
                return false;
        }
    }
    offsets[MG_WB_STATES] = at;
    if (!mg_wb_add(&at, w * n_jobs, sizeof(mg_walk_state))) return false;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        offsets[MG_WB_OFF(g, MG_WB_DESTS)] = at;
        if (!mg_wb_add(&at, w * shapes[g].n_slots, 4)) return false;
    }
    offsets[MG_WB_ROOTBITS] = at;
    if (!mg_wb_add(&at, (total + 63) / 64 * n_jobs, 8)) return false;
    /* rows of 8 limbs x total lanes; total < 2^26, so rows x total fits */
    uint64_t leaf_b = 0, probe_b = 0;
    if (!mg_wb_add(&leaf_b, (uint64_t)max_leaves * total, 32)) return false;
    if (!mg_wb_add(&probe_b, (uint64_t)max_probes * total, 32)) return false;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        offsets[MG_WB_OFF(g, MG_WB_LEAVES)] = at;
        if (__builtin_add_overflow(at, leaf_b, &at)) return false;
    }
    for (uint32_t g = 0; g < n_jobs; ++g) {
        offsets[MG_WB_OFF(g, MG_WB_PROBES)] = at;
        if (__builtin_add_overflow(at, probe_b, &at)) return false;
    }
    *bytes = at;
    if (leaf_stride_w) *leaf_stride_w = leaf_b / 4;
    if (probe_stride_w) *probe_stride_w = probe_b / 4;
    return true;
}

#endif

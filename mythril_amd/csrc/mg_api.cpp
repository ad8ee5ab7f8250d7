// C ABI of libmythgpu (include/mythgpu.h).  Host-side validation, device
// memory management and kernel launches.  Every program is validated before
// upload so that no instruction can index outside the register file, the LDS
// spill area, the constant pool, the leaf table or the probe buffer.

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <algorithm>
#include <vector>

#include <cstddef>
#include <cstdlib>
#include <map>
#include <elf.h>
#include <dlfcn.h>

#include "mythgpu.h"
#include "mythgpu_ir.h"
#include "mg_device.h"
#include "mg_asm_handlers.h"
#include "mg_host.h"
#include "mg_census.h"
#include "mg_census_batch.h"
#include "mg_repair.h"
#include "mg_walk.h"
#include "mg_walk_tree.h"
#include "mg_walk_aim.h"
#include "mg_walk_sum.h"
#include "mg_walk_batch.h"
#include "mg_carry.h"

// the interpreter of each register layout (mg_interp_asm.hip, one
// translation unit per layout; mg_find_layout lists them)
typedef hipError_t (*mg_launch_fn)(const mg_pdesc* d_descs, uint32_t n_progs, const mg_run& run,
                                   uint32_t mode, uint32_t lds_slots, uint32_t* table,
                                   hipStream_t stream);
hipError_t mg_launch_asm_r16(const mg_pdesc*, uint32_t, const mg_run&, uint32_t, uint32_t, uint32_t*,
                             hipStream_t);
hipError_t mg_launch_asm_r11(const mg_pdesc*, uint32_t, const mg_run&, uint32_t, uint32_t, uint32_t*,
                             hipStream_t);
const char* mg_asm_digest_r16(void);
const char* mg_asm_digest_r11(void);
static_assert(MG_NREG == 16 && MG_NREG_W4 == 11, "one interpreter per layout: _r16, _r11");

static mg_launch_fn layout_launch(uint32_t nreg) {
    return nreg == MG_NREG_W4 ? mg_launch_asm_r11 : mg_launch_asm_r16;
}

hipError_t mg_launch_keccak(const uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len,
                            uint32_t n, uint8_t* d_out, hipStream_t stream);
// verdict census of one chunk's mask probes (mg_census.hip; counter block of
// mg_census.h): rows = the first mask probe's rows, n <= stride lanes,
// candidate indices first.., offsets offset.. from the census's first index
hipError_t mg_launch_census(const uint32_t* d_rows, uint64_t stride, uint64_t n, uint32_t n_roots,
                            uint64_t first, uint64_t offset, unsigned long long* d_out,
                            hipStream_t stream);
// one round of the local search (mg_repair.hip): the neighbours of the base
// into the interpreter's eval-mode input; then, after the interpreter wrote
// their verdict masks (rows = the first mask probe's rows, stride lanes), the
// best neighbour into the base and its failing roots into trace[r]
hipError_t mg_launch_census_batch(const mg_census_batch_job* d_jobs, uint32_t n_jobs,
                                  uint64_t stride, uint64_t n, uint64_t first, uint64_t offset,
                                  hipStream_t stream);
hipError_t mg_launch_repair_round(uint32_t* d_base, const mg_leafgen* d_gen,
                                  const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                                  uint32_t r, uint32_t lanes, uint32_t* d_leaves,
                                  hipStream_t stream);
hipError_t mg_launch_repair_pick(const uint32_t* d_rows, uint32_t lanes, uint32_t n_roots,
                                 uint32_t* d_base, const mg_leafgen* d_gen,
                                 const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                                 uint32_t r, mg_repair_state* d_state, uint32_t* d_trace,
                                 hipStream_t stream);
// one round of the scored walk (mg_walk.hip), all walkers per launch: the
// neighbours of every base into the eval-mode input ([..][walkers * lanes]);
// then, after the interpreter wrote their masks and residual probes, each
// walker's best neighbour into its base and its key into trace[w][r]
hipError_t mg_launch_walk_round(const uint32_t* d_bases, const mg_leafgen* d_gen,
                                const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                                uint32_t r, uint32_t lanes, uint32_t walkers, uint32_t* d_leaves,
                                hipStream_t stream);
hipError_t mg_launch_walk_pick(const uint32_t* d_masks, const uint32_t* d_resid,
                               const uint32_t* d_table, uint32_t lanes, uint32_t walkers,
                               uint32_t n_roots, uint32_t* d_bases, const mg_leafgen* d_gen,
                               const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                               uint32_t r, uint32_t max_rounds, mg_walk_state* d_state,
                               uint32_t* d_trace, hipStream_t stream);
// the same round with the tree scoring (mg_walk_tree.hip): the score kernel of
// DESIGN.md §3.11, then the adopt step of mg_walk.hip
hipError_t mg_launch_walk_tree_pick(const uint32_t* d_masks, const uint32_t* d_amasks,
                                    const uint32_t* d_resid, const uint32_t* d_roots,
                                    const uint32_t* d_atoms, const uint32_t* d_code,
                                    uint32_t lanes, uint32_t walkers, uint32_t n_roots,
                                    uint32_t* d_bases, const mg_leafgen* d_gen,
                                    const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                                    uint32_t r, uint32_t max_rounds, mg_walk_state* d_state,
                                    uint32_t* d_trace, hipStream_t stream);
// the round of mg_walk_aim (mg_walk_aim.hip): the mutate and
// the adopt step know the aim table; the score kernel is mg_walk_tree's
hipError_t mg_launch_walk_aim_round(const uint32_t* d_bases, const mg_leafgen* d_gen,
                                    const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                                    uint32_t r, uint32_t lanes, uint32_t walkers,
                                    const uint32_t* d_entries, uint32_t n_entries,
                                    const uint32_t* d_pieces, const uint32_t* d_rstate,
                                    uint32_t n_resid, const uint32_t* d_lives, uint32_t* d_leaves,
                                    hipStream_t stream);
hipError_t mg_launch_walk_aim_pick(const uint32_t* d_masks, const uint32_t* d_amasks,
                                   const uint32_t* d_resid, const uint32_t* d_roots,
                                   const uint32_t* d_atoms, const uint32_t* d_code, uint32_t lanes,
                                   uint32_t walkers, uint32_t n_roots, uint32_t* d_bases,
                                   const mg_leafgen* d_gen, const uint32_t* d_consts,
                                   uint32_t n_leaves, uint64_t seed, uint32_t r,
                                   uint32_t max_rounds, const uint32_t* d_entries,
                                   uint32_t n_entries, const uint32_t* d_pieces, uint32_t n_resid,
                                   uint32_t* d_rstate, uint32_t* d_lives, mg_walk_state* d_state,
                                   uint32_t* d_trace, hipStream_t stream);
// the round of mg_walk_bound, mg_walk_uf and mg_walk_sum (mg_walk_sum.hip,
// DESIGN.md §3.13 - §3.15): mg_walk_aim's with the wider table, the side's
// fixed bits and the walkers' mask state; the walkers' slot destinations, U
// rows and the UF tables; the entries' lin words and the walkers' side rows.
// A lower rung passes lin words all 0 and empty tables.
hipError_t mg_launch_walk_sum_round(const uint32_t* d_bases, const mg_leafgen* d_gen,
                                    const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                                    uint32_t r, uint32_t lanes, uint32_t walkers,
                                    const uint32_t* d_entries, uint32_t n_entries,
                                    const uint32_t* d_pieces, const uint32_t* d_fixed,
                                    const uint32_t* d_lin, const uint32_t* d_rstate,
                                    uint32_t n_resid, const uint32_t* d_sstate, uint32_t n_srows,
                                    const uint32_t* d_lives, const uint32_t* d_dests,
                                    uint32_t n_slots, uint32_t* d_leaves, hipStream_t stream);
hipError_t mg_launch_walk_sum_pick(const uint32_t* d_masks, const uint32_t* d_amasks,
                                   const uint32_t* d_resid, const uint32_t* d_srows,
                                   uint32_t n_srows, const uint32_t* d_urows,
                                   const uint32_t* d_roots, const uint32_t* d_atoms,
                                   const uint32_t* d_code, uint32_t lanes, uint32_t walkers,
                                   uint32_t n_roots, uint32_t n_atoms, uint32_t* d_bases,
                                   const mg_leafgen* d_gen, const uint32_t* d_consts,
                                   uint32_t n_leaves, uint64_t seed, uint32_t r,
                                   uint32_t max_rounds, const uint32_t* d_entries,
                                   uint32_t n_entries, const uint32_t* d_pieces,
                                   const uint32_t* d_fixed, const uint32_t* d_lin,
                                   uint32_t n_resid, const mg_uf_tables& uf, uint32_t* d_rstate,
                                   uint32_t* d_mstate, uint32_t* d_sstate, uint32_t* d_ustate,
                                   uint32_t* d_dests, uint32_t* d_lives, mg_walk_state* d_state,
                                   uint32_t* d_trace, hipStream_t stream);


hipError_t mg_launch_walk_batch_round(const mg_walk_batch_job* d_jobs, const uint32_t* d_frozen,
                                     uint32_t n_jobs, uint32_t r, uint32_t lanes,
                                     uint32_t walkers, uint32_t max_rounds, hipStream_t stream);
hipError_t mg_launch_walk_batch_pick(const mg_walk_batch_job* d_jobs, const uint32_t* d_frozen,
                                    uint32_t n_jobs, uint32_t r, uint32_t lanes, uint32_t walkers,
                                    uint32_t max_rounds, hipStream_t stream);

// the two kernels around mg_carry_batch's interpreter launch (mg_carry.hip)
hipError_t mg_launch_carry_fill(const mg_carry_dev_job* d_jobs, uint32_t n_jobs,
                                uint32_t most_leaves, uint64_t seed, uint64_t first_index,
                                uint32_t lanes, hipStream_t stream);
hipError_t mg_launch_carry_gather(const mg_carry_dev_job* d_jobs, uint32_t n_jobs,
                                  const unsigned long long* d_first, uint32_t lanes,
                                  uint32_t max_leaves, long long* d_out_first,
                                  uint32_t* d_out_leaves, hipStream_t stream);
// the two around mg_carry_ladder's (mg_carry_ladder.hip)
hipError_t mg_launch_carry_fill_rungs(const mg_carry_dev_job* d_jobs, uint32_t n_jobs,
                                      uint32_t most_leaves, uint64_t seed, uint64_t first_index,
                                      uint32_t lanes, uint32_t cols, hipStream_t stream);
hipError_t mg_launch_carry_gather_rungs(const mg_carry_dev_job* d_jobs, uint32_t n_jobs,
                                        const unsigned long long* d_first, uint32_t lanes,
                                        uint32_t cols, uint32_t max_leaves,
                                        long long* d_out_first, long long* d_out_rung,
                                        uint32_t* d_out_leaves, hipStream_t stream);
// the fill of mg_carry_ladder_sets (mg_carry_sets.hip); its gather is the ladder's
hipError_t mg_launch_carry_fill_sets(const mg_carry_dev_job* d_jobs,
                                     const mg_carry_sets_dev_job* d_sjobs, uint32_t n_jobs,
                                     uint32_t most_leaves, uint64_t seed, uint64_t first_index,
                                     uint32_t lanes, uint32_t cols, hipStream_t stream);
// the two after mg_carry_census's (mg_carry_census.hip)
hipError_t mg_launch_carry_census(const mg_carry_dev_job* d_jobs,
                                  const mg_carry_census_dev_job* d_cjobs, uint32_t n_jobs,
                                  uint32_t rungs, uint32_t lanes, uint32_t cols,
                                  hipStream_t stream);
hipError_t mg_launch_carry_starts(const mg_carry_dev_job* d_jobs,
                                  const mg_carry_census_dev_job* d_cjobs, uint32_t n_jobs,
                                  uint32_t walkers, uint32_t cols, uint32_t max_leaves,
                                  long long* d_out_col, uint32_t* d_out_nfail,
                                  uint32_t* d_out_rows, hipStream_t stream);
static_assert(MG_CARRY_MAX_WALKERS == MG_WALK_MAX_WALKERS,
              "mg_carry_census hands its starts to the walks");

struct mg_ctx {
    int device = 0;
    // register layout of this context's interpreter (mg_init_layout): its
    // slot count, kernel and LDS spill regions per lane (the layout's default
    // — 6 fill the CU at three 256-lane blocks, 13 halves; 5 at four blocks —
    // unless MYTHGPU_LDS_SLOTS sets it)
    uint32_t nreg = MG_NREG;
    mg_launch_fn launch_asm = mg_launch_asm_r16;
    hipStream_t stream = nullptr;
    std::string err;
    char name[256] = {0};
    int cus = 0;
    // assembly interpreter: handler byte offsets (query launch at init) and
    // LDS spill slots per 256-lane block
    uint32_t hoff[MGA_NUM_HANDLERS] = {0};
    uint32_t lds_slots = 6;
    // generator boundary-value table (device, 48 KiB; MG_BTAB_WORDS)
    uint32_t* d_btab = nullptr;
    // grow-only device workspace for synchronous calls
    void* ws = nullptr;
    size_t ws_size = 0;
    // device time of the last synchronous eval / search (HIP events around
    // its launches on the context stream; mg_last_kernel_ms)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.f;
    // device blocks of programs and batches (dev_alloc): power-of-two size
    // classes; classes below MG_SLAB_CLASS_MAX are carved from slabs, larger
    // ones are whole allocations; freed blocks wait on a per-class list, so
    // a get_model query's loads and frees make no hipMalloc / hipFree (each
    // costs tens of microseconds, and hipFree synchronises the device)
    std::map<size_t, std::vector<void*>> free_blocks;
    std::vector<void*> slabs, large;
    uint8_t* slab_cur = nullptr;
    size_t slab_left = 0;
    // the last launch on each caller stream (mg_batch_eval_gen), one event
    // per stream: a freed block is reused only after every launch that
    // might read it completed, on whichever streams they were queued
    struct ext_stream { hipStream_t stream; hipEvent_t ev; bool pending; };
    std::vector<ext_stream> ext;
    // pinned host staging for program uploads (grow-only): the blob is
    // assembled in place and copied at pinned-DMA rate; a leaf-pool-heavy
    // search program is ~1 MB (the pools' (v-1, v, v+1) triples)
    uint8_t* h_stage = nullptr;
    size_t h_stage_size = 0;
};

static void timing_begin(mg_ctx* ctx) {
    ctx->last_ms = 0.f;
    if (ctx->ev0) (void)hipEventRecord(ctx->ev0, ctx->stream);
}

static void timing_end(mg_ctx* ctx) {
    if (ctx->ev1) (void)hipEventRecord(ctx->ev1, ctx->stream);
}

// after the stream was synchronised
static void timing_read(mg_ctx* ctx) {
    float ms = 0.f;
    if (ctx->ev0 && ctx->ev1 && hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess)
        ctx->last_ms = ms;
}

struct mg_jit;

struct mg_prog {
    mg_ctx* ctx = nullptr;
    mg_jit* jit = nullptr;          // the compiled-program image it is attached to
    void* d_blob = nullptr;         // code | consts | gen | desc | xcode
    size_t blob_cls = 0;            // its dev_alloc size class
    mg_pdesc* d_desc = nullptr;
    mg_pdesc h_desc;                // host copy (batches copy it from here)
    uint32_t n_ins = 0, n_consts = 0, n_leaves = 0, n_lds = 0, n_probes = 0;
    uint64_t rec_fp = 0;            // records' fingerprint (rec_fingerprint)
    std::vector<mg_leafgen> leafgen;   // as loaded (mg_repair's move function reads it)
};

// Fingerprint of a program's records with HANDLER IDS in word 0 (the
// translator run with the identity table, before word 0 becomes this
// library's handler offset): every word times successive powers of
// 0x100000001B3 mod 2^64, plus the record count (mythril_amd/jit.py
// records_fingerprint).  The handler id names the operation and its variant,
// so two programs whose records differ only in an opcode (ADD / SUB, ULT /
// SLT) differ here.  A compiled-program image carries it per entry, so
// mg_jit_attach refuses code built for other records.
static uint64_t rec_fingerprint(const std::vector<uint32_t>& rec) {
    uint64_t h = 0, p = 1;
    for (size_t r = 0; r + 8 <= rec.size(); r += 8)
        for (int k = 0; k < 8; ++k) {
            p *= 0x100000001B3ull;
            h += (uint64_t)rec[r + k] * p;
        }
    return h + rec.size() / 8;
}

// The identity handler table: the translator then writes handler ids into
// word 0 (fingerprinted, then mapped through the context's offsets).
// Built once by a function-local static (thread-safe initialisation: two
// contexts may load programs from two host threads at once).
static const uint32_t* identity_handlers() {
    struct table {
        uint32_t t[MGA_NUM_HANDLERS];
        table() {
            for (uint32_t h = 0; h < MGA_NUM_HANDLERS; ++h) t[h] = h;
        }
    };
    static const table tab;
    return tab.t;
}

static uint32_t kernel_lds_slots(const mg_ctx* ctx, uint32_t n_lds) {
    return n_lds < ctx->lds_slots ? n_lds : ctx->lds_slots;
}

static hipError_t launch(const mg_ctx* ctx, int gen, const mg_pdesc* d_descs, uint32_t n_progs,
                         const mg_run& run, uint32_t n_lds, hipStream_t stream) {
    return ctx->launch_asm(d_descs, n_progs, run, gen ? 1u : 0u, kernel_lds_slots(ctx, n_lds),
                           nullptr, stream);
}

// A loaded compiled-program code object (mythril_amd/jit.py) and the
// programs whose descriptors point into it.
struct mg_jit {
    mg_ctx* ctx = nullptr;
    hipModule_t module = nullptr;
    std::vector<mg_prog*> progs;
};

struct mg_batch {
    mg_ctx* ctx = nullptr;
    mg_pdesc* d_descs = nullptr;
    size_t descs_cls = 0;
    uint32_t n = 0;
    uint32_t max_lds = 0;
    uint32_t max_leaves = 0;
    uint32_t max_probes = 0;
};

static int fail(mg_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

#define HIPCHECK(ctx, expr)                                                              \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return fail(ctx, MG_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                        __FILE__, __LINE__);                                            \
    } while (0)

#define MG_SLAB_BYTES ((size_t)4 << 20)
#define MG_SLAB_CLASS_MAX ((size_t)256 << 10)
#define MG_BLOCK_MIN ((size_t)4 << 10)

static size_t block_class(size_t bytes) {
    size_t c = MG_BLOCK_MIN;
    while (c < bytes) c <<= 1;
    return c;
}

// A device block of at least `bytes` (256-byte aligned); *cls receives its
// size class for dev_release.
static hipError_t dev_alloc(mg_ctx* ctx, size_t bytes, void** out, size_t* cls) {
    const size_t c = block_class(bytes);
    *cls = c;
    auto it = ctx->free_blocks.find(c);
    if (it != ctx->free_blocks.end() && !it->second.empty()) {
        *out = it->second.back();
        it->second.pop_back();
        return hipSuccess;
    }
    if (c > MG_SLAB_CLASS_MAX) {
        hipError_t e = hipMalloc(out, c);
        if (e == hipSuccess) ctx->large.push_back(*out);
        return e;
    }
    if (ctx->slab_left < c) {
        void* slab = nullptr;
        hipError_t e = hipMalloc(&slab, MG_SLAB_BYTES);
        if (e != hipSuccess) return e;
        ctx->slabs.push_back(slab);
        ctx->slab_cur = (uint8_t*)slab;
        ctx->slab_left = MG_SLAB_BYTES;
    }
    *out = ctx->slab_cur;                   // classes are powers of two <= the slab
    ctx->slab_cur += c;
    ctx->slab_left -= c;
    return hipSuccess;
}

// Back to its class list once no queued launch can still read it: the
// context stream and the last launch on every caller stream are waited for
// (what the hipFree this replaces did by synchronising the device).
static void dev_release(mg_ctx* ctx, void* p, size_t cls) {
    if (!p) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& x : ctx->ext)
        if (x.pending) {
            (void)hipEventSynchronize(x.ev);
            x.pending = false;
        }
    ctx->free_blocks[cls].push_back(p);
}

// Note a launch on a caller stream (its event is recorded after it).
static hipError_t ext_launched(mg_ctx* ctx, hipStream_t s) {
    for (auto& x : ctx->ext)
        if (x.stream == s) {
            x.pending = true;
            return hipEventRecord(x.ev, s);
        }
    hipEvent_t ev = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess)                   // no event: wait now; nothing stays pending
        return hipStreamSynchronize(s);
    ctx->ext.push_back({s, ev, true});
    return hipEventRecord(ev, s);
}

static int workspace(mg_ctx* ctx, size_t bytes, void** out) {
    if (bytes > ctx->ws_size) {
        if (ctx->ws) (void)hipFree(ctx->ws);
        ctx->ws = nullptr;
        ctx->ws_size = 0;
        size_t sz = bytes < (1u << 20) ? (1u << 20) : bytes;
        HIPCHECK(ctx, hipMalloc(&ctx->ws, sz));
        ctx->ws_size = sz;
    }
    *out = ctx->ws;
    return MG_OK;
}


// One launch in query mode: the assembly interpreter writes the byte offset
// of every handler (relative to its dispatch base) into a table.
static int query_handlers(mg_ctx* ctx) {
    void* d = nullptr;
    const size_t tab_b = sizeof(uint32_t) * MGA_NUM_HANDLERS;
    HIPCHECK(ctx, hipMalloc(&d, tab_b + 256));
    mg_pdesc* d_desc = (mg_pdesc*)((uint8_t*)d + tab_b);
    mg_pdesc zero;
    memset(&zero, 0, sizeof zero);
    zero.consts = (const uint32_t*)d;
    zero.xcode = (const uint32_t*)d;
    hipError_t e = hipMemcpy(d_desc, &zero, sizeof zero, hipMemcpyHostToDevice);
    mg_run run;
    memset(&run, 0, sizeof run);
    run.n_assign = 1;
    run.stride = 1;
    if (e == hipSuccess) e = ctx->launch_asm(d_desc, 1, run, 2u, 0, (uint32_t*)d, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->hoff, d, tab_b, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(ctx, MG_E_HIP, "handler query: %s", hipGetErrorString(e));
    for (int h = 0; h < MGA_NUM_HANDLERS; ++h)
        if (ctx->hoff[h] == 0 || ctx->hoff[h] > (1u << 24))
            return fail(ctx, MG_E_HIP, "handler query: bad offset %u for %d", ctx->hoff[h], h);
    return MG_OK;
}

extern "C" {


// Boundary values of the candidate generator as a table the LEAF handler
// indexes by kind * 256 + p (oracle/gen_ref.py gen_leaf, boundary class):
// kind 0: 0, 1: 1, 2: 1 << p (p = width - 1), 3: 2^256 - 1, 4: (1 << p) + 1,
// 5: (1 << p) - 1 (p = k); the handler masks to the width afterwards.
#define MG_BTAB_WORDS (6 * 256 * 8)
static void mg_boundary_table(uint32_t* t) {
    memset(t, 0, MG_BTAB_WORDS * 4);
    for (uint32_t p = 0; p < 256; ++p) {
        uint32_t* e1 = t + (1 * 256 + p) * 8;
        uint32_t* e2 = t + (2 * 256 + p) * 8;
        uint32_t* e3 = t + (3 * 256 + p) * 8;
        uint32_t* e4 = t + (4 * 256 + p) * 8;
        uint32_t* e5 = t + (5 * 256 + p) * 8;
        e1[0] = 1;
        e2[p >> 5] = 1u << (p & 31);
        for (int j = 0; j < 8; ++j) e3[j] = ~0u;
        e4[p >> 5] = 1u << (p & 31);
        e4[0] += 1;                              // p = 0: 1 + 1 = 2
        for (uint32_t j = 0; j < (p >> 5); ++j) e5[j] = ~0u;
        e5[p >> 5] = (1u << (p & 31)) - 1;
    }
}

int mg_init(int device, mg_ctx** out) { return mg_init_layout(device, MG_NREG, out); }

const char* mg_asm_digest(void) { return mg_asm_digest_r16(); }

const char* mg_asm_digest_layout(uint32_t nreg) {
    if (nreg == MG_NREG) return mg_asm_digest_r16();
    if (nreg == MG_NREG_W4) return mg_asm_digest_r11();
    return nullptr;
}

int mg_init_layout(int device, uint32_t nreg, mg_ctx** out) {
    if (!out) return MG_E_ARG;
    *out = nullptr;
    const mg_layout_info* lay = mg_find_layout(nreg);
    if (!lay) return MG_E_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return MG_E_NODEV;
    if (device < 0 || device >= n) return MG_E_NODEV;
    mg_ctx* ctx = new mg_ctx();
    ctx->device = device;
    ctx->nreg = nreg;
    ctx->launch_asm = layout_launch(nreg);
    ctx->lds_slots = lay->lds_slots;
    if (hipSetDevice(device) != hipSuccess) {
        delete ctx;
        return MG_E_NODEV;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        snprintf(ctx->name, sizeof ctx->name, "%s (%s)", prop.name, prop.gcnArchName);
        ctx->cus = prop.multiProcessorCount;
    }
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return MG_E_HIP;
    }
    if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) {
        mg_free(ctx);
        return MG_E_HIP;
    }
    if (const char* l = getenv("MYTHGPU_LDS_SLOTS")) {
        // a region count whose halves a DS offset cannot reach is refused
        // here, not found later by the assembler
        char* end = nullptr;
        const long v = strtol(l, &end, 10);
        if (end == l || *end || v < 0 || v > MG_MAX_LDS_DS) {
            mg_free(ctx);
            return MG_E_ARG;
        }
        ctx->lds_slots = (uint32_t)v;
    }
    if (query_handlers(ctx) != MG_OK) {
        mg_free(ctx);
        return MG_E_HIP;
    }
    {
        std::vector<uint32_t> bt(MG_BTAB_WORDS);
        mg_boundary_table(bt.data());
        if (hipMalloc(&ctx->d_btab, MG_BTAB_WORDS * 4) != hipSuccess ||
            hipMemcpy(ctx->d_btab, bt.data(), MG_BTAB_WORDS * 4, hipMemcpyHostToDevice) !=
                hipSuccess) {
            mg_free(ctx);
            return MG_E_HIP;
        }
    }
    *out = ctx;
    return MG_OK;
}

void mg_free(mg_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->ws) (void)hipFree(ctx->ws);
    if (ctx->d_btab) (void)hipFree(ctx->d_btab);
    for (void* q : ctx->slabs) (void)hipFree(q);
    for (void* q : ctx->large) (void)hipFree(q);
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    for (auto& x : ctx->ext) {
        (void)hipEventSynchronize(x.ev);
        (void)hipEventDestroy(x.ev);
    }
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int mg_runtime_info(int* hip_version, char* path, size_t path_len) {
    if (hip_version) {
        *hip_version = 0;
        if (hipRuntimeGetVersion(hip_version) != hipSuccess) *hip_version = 0;
    }
    if (path && path_len) {
        path[0] = 0;
        Dl_info info;
        if (dladdr((void*)&hipRuntimeGetVersion, &info) && info.dli_fname)
            snprintf(path, path_len, "%s", info.dli_fname);
    }
    return MG_OK;
}

const char* mg_last_error(const mg_ctx* ctx) { return ctx ? ctx->err.c_str() : "no context"; }

float mg_last_kernel_ms(const mg_ctx* ctx) { return ctx ? ctx->last_ms : 0.f; }

int mg_device_info(mg_ctx* ctx, char* name, size_t name_len, int* n_cus) {
    if (!ctx) return MG_E_ARG;
    if (name && name_len) snprintf(name, name_len, "%s", ctx->name);
    if (n_cus) *n_cus = ctx->cus;
    return MG_OK;
}

int mg_load_program(mg_ctx* ctx, const uint32_t* code, uint32_t n_ins, const uint32_t* consts,
                    uint32_t n_consts, const mg_leafgen* leaves, uint32_t n_leaves,
                    uint32_t n_spill_slots, uint32_t n_probes, uint64_t prog_seed,
                    mg_prog** out) {
    if (!ctx || !out || (n_ins && !code) || (n_consts && !consts) || (n_leaves && !leaves))
        return fail(ctx, MG_E_ARG, "null argument");
    *out = nullptr;
    const uint32_t n_lds_slots = n_spill_slots < MG_MAX_LDS ? n_spill_slots : MG_MAX_LDS;
    int rc = mg_validate(ctx ? &ctx->err : nullptr, code, n_ins, n_consts, leaves, n_leaves, n_lds_slots, n_spill_slots,
                         n_probes, ctx->nreg);
    if (rc) return rc;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    // assembly records + translator masks (appended to the constant table);
    // word 0 holds handler ids until the fingerprint is taken
    std::vector<uint32_t> rec;
    MaskPool pool;
    mg_translate_records(identity_handlers(), code, n_ins, n_consts,
                         kernel_lds_slots(ctx, n_spill_slots), ctx->nreg, rec, pool);
    const uint32_t n_masks = (uint32_t)(pool.words.size() / 8);
    const uint32_t n_const_all = n_consts + n_masks + n_consts * 3;
    // device leaf descriptors: byte pool offsets and the per-leaf stream salt
    std::vector<mg_leafgen_dev> gdev(n_leaves);
    for (uint32_t i = 0; i < n_leaves; ++i) {
        const uint64_t salt = (prog_seed * 0xD1B54A32D192ED03ull) ^
                              ((uint64_t)(i + 1) * 0x8CB92BA72F3D8DD7ull);
        gdev[i] = {leaves[i].width, (n_consts + n_masks + 3 * leaves[i].pool_off) * 32u,
                   leaves[i].pool_n,
                   leaves[i].pct_uniform, leaves[i].pct_small, leaves[i].pct_boundary,
                   (uint32_t)salt, (uint32_t)(salt >> 32)};
    }
    // LEAFD records carry their leaf's generator parameters (asmgen.py
    // LEAFD_*: no descriptor load in the handler): pool offset, salt, pool
    // size and the class thresholds packed one per byte
    for (size_t r = 0; r + 8 <= rec.size(); r += 8) {
        if (rec[r] >= MGA_NUM_HANDLERS || rec[r] / (2 * MGA_NVAR) != MGA_LEAFD) continue;
        const uint32_t li = rec[r + 4];
        if (li >= n_leaves) continue;            // eval mode only (no generator)
        const mg_leafgen_dev& g = gdev[li];
        rec[r + 1] = g.pool_off_b;
        rec[r + 2] = g.salt_lo;
        rec[r + 3] = g.salt_hi;
        rec[r + 5] = g.pool_n;
        rec[r + 7] = g.pct_uniform | g.pct_small << 8 | g.pct_boundary << 16;
    }
    const uint64_t rec_fp = rec_fingerprint(rec);
    // handler ids -> this library's handler offsets (the zeroed pad record
    // stays zero)
    for (size_t r = 0; r + 8 <= rec.size(); r += 8)
        if (r + 8 < rec.size() || rec[r] != 0) rec[r] = ctx->hoff[rec[r] % MGA_NUM_HANDLERS];
    // 8 zeroed NOPs after the IR code: the C++ interpreter prefetches ahead
    const size_t code_b = (size_t)(n_ins + 8) * 16, const_b = (size_t)n_const_all * 32,
                 gen_b = gdev.size() * sizeof(mg_leafgen_dev), rec_b = rec.size() * 4;
    auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t off_const = align(code_b), off_gen = off_const + align(const_b),
                 off_desc = off_gen + align(gen_b), off_rec = off_desc + align(sizeof(mg_pdesc)),
                 total = off_rec + align(rec_b);
    if (total > ctx->h_stage_size) {
        if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
        ctx->h_stage = nullptr;
        ctx->h_stage_size = 0;
        size_t sz = (size_t)4 << 20;
        while (sz < total) sz <<= 1;
        HIPCHECK(ctx, hipHostMalloc((void**)&ctx->h_stage, sz, hipHostMallocDefault));
        ctx->h_stage_size = sz;
    }
    uint8_t* blob = ctx->h_stage;   // free: every upload below is synchronous
    memset(blob, 0, total);
    if (n_ins) memcpy(blob, code, (size_t)n_ins * 16);   // + zeroed NOP padding
    if (n_consts) memcpy(blob + off_const, consts, (size_t)n_consts * 32);
    if (!pool.words.empty())
        memcpy(blob + off_const + (size_t)n_consts * 32, pool.words.data(), pool.words.size() * 4);
    // generator pools expanded to (v - 1, v, v + 1) triples (mod 2^256), so
    // the pool class is one indexed load (pool[e] + delta - 1, gen_ref.py)
    {
        uint32_t* pm = (uint32_t*)(blob + off_const + (size_t)(n_consts + n_masks) * 32);
        for (uint32_t c = 0; c < n_consts; ++c) {
            const uint32_t* v = consts + (size_t)c * 8;
            uint32_t* o = pm + (size_t)c * 24;
            uint64_t bm = 1, bp = 1;             // borrow of v - 1, carry of v + 1
            for (int j = 0; j < 8; ++j) {
                o[j] = v[j] - (uint32_t)bm;
                bm = bm && v[j] == 0;
                o[8 + j] = v[j];
                o[16 + j] = v[j] + (uint32_t)bp;
                bp = bp && v[j] == 0xFFFFFFFFu;
            }
        }
    }
    if (gen_b) memcpy(blob + off_gen, gdev.data(), gen_b);
    memcpy(blob + off_rec, rec.data(), rec_b);
    void* d = nullptr;
    size_t cls = 0;
    HIPCHECK(ctx, dev_alloc(ctx, total, &d, &cls));
    uint8_t* db = (uint8_t*)d;
    mg_pdesc desc;
    memset(&desc, 0, sizeof desc);
    desc.code = (const uint32_t*)db;
    desc.consts = (const uint32_t*)(db + off_const);
    desc.gen = (const mg_leafgen_dev*)(db + off_gen);
    desc.n_ins = n_ins;
    desc.n_leaves = n_leaves;
    desc.n_lds = n_lds_slots;
    desc.n_probes = n_probes;
    desc.prog_seed = prog_seed;
    desc.xcode = (const uint32_t*)(db + off_rec);
    desc.btab = ctx->d_btab;
    memcpy(blob + off_desc, &desc, sizeof desc);
    hipError_t e = hipMemcpyAsync(d, blob, total, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        dev_release(ctx, d, cls);
        return fail(ctx, MG_E_HIP, "upload: %s", hipGetErrorString(e));
    }
    mg_prog* p = new mg_prog();
    p->ctx = ctx;
    p->rec_fp = rec_fp;
    p->d_blob = d;
    p->blob_cls = cls;
    p->d_desc = (mg_pdesc*)(db + off_desc);
    p->h_desc = desc;
    p->n_ins = n_ins;
    p->n_consts = n_consts;
    p->n_leaves = n_leaves;
    p->n_lds = n_lds_slots;
    p->n_probes = n_probes;
    p->leafgen.assign(leaves, leaves + n_leaves);
    *out = p;
    return MG_OK;
}

void mg_free_program(mg_prog* p) {
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    if (p->jit) {                   // a later detach must not write into a reused block
        auto& v = p->jit->progs;
        v.erase(std::remove(v.begin(), v.end(), p), v.end());
    }
    dev_release(p->ctx, p->d_blob, p->blob_cls);
    delete p;
}

static mg_run empty_run() {
    mg_run r;
    memset(&r, 0, sizeof r);
    return r;
}

int mg_eval(mg_ctx* ctx, const mg_prog* prog, const uint32_t* leaves_soa, uint64_t n_assign,
            uint64_t* root_bits, uint32_t* probes) {
    if (!ctx || !prog || !root_bits || (prog->n_leaves && !leaves_soa))
        return fail(ctx, MG_E_ARG, "null argument");
    if (n_assign == 0) return MG_OK;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    const uint64_t words = (n_assign + 63) / 64;
    const size_t leaf_b = (size_t)prog->n_leaves * 8 * n_assign * 4;
    const size_t probe_b = probes ? (size_t)prog->n_probes * 8 * n_assign * 4 : 0;
    const size_t root_b = words * 8;
    void* ws;
    int rc = workspace(ctx, leaf_b + probe_b + root_b + 256, &ws);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)ws;
    mg_run run = empty_run();
    run.leaves = (const uint32_t*)base;
    run.root_bits = (uint64_t*)(base + leaf_b);
    run.probes = probes ? (uint32_t*)(base + leaf_b + root_b) : nullptr;
    run.stride = n_assign;
    run.n_assign = n_assign;
    run.words_per_prog = words;
    if (leaf_b)
        HIPCHECK(ctx, hipMemcpyAsync(base, leaves_soa, leaf_b, hipMemcpyHostToDevice, ctx->stream));
    timing_begin(ctx);
    HIPCHECK(ctx, launch(ctx, 0, prog->d_desc, 1, run, prog->n_lds, ctx->stream));
    timing_end(ctx);
    HIPCHECK(ctx, hipMemcpyAsync(root_bits, run.root_bits, root_b, hipMemcpyDeviceToHost,
                                 ctx->stream));
    if (probes && probe_b)
        HIPCHECK(ctx, hipMemcpyAsync(probes, run.probes, probe_b, hipMemcpyDeviceToHost,
                                     ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    timing_read(ctx);
    return MG_OK;
}

int mg_eval_gen(mg_ctx* ctx, const mg_prog* prog, const mg_gen* gen, uint64_t n_assign,
                uint64_t* root_bits, uint32_t* probes, uint32_t* leaves_out) {
    if (!ctx || !prog || !gen || !root_bits) return fail(ctx, MG_E_ARG, "null argument");
    if (n_assign == 0) return MG_OK;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    const uint64_t words = (n_assign + 63) / 64;
    const size_t leaf_b = leaves_out ? (size_t)prog->n_leaves * 8 * n_assign * 4 : 0;
    const size_t probe_b = probes ? (size_t)prog->n_probes * 8 * n_assign * 4 : 0;
    const size_t root_b = words * 8;
    void* ws;
    int rc = workspace(ctx, leaf_b + probe_b + root_b + 256, &ws);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)ws;
    mg_run run = empty_run();
    run.root_bits = (uint64_t*)base;
    run.probes = probes ? (uint32_t*)(base + root_b) : nullptr;
    run.leaves_out = leaves_out ? (uint32_t*)(base + root_b + probe_b) : nullptr;
    run.stride = n_assign;
    run.n_assign = n_assign;
    run.words_per_prog = words;
    run.seed = gen->seed;
    run.first_index = gen->first_index;
    if (leaf_b) HIPCHECK(ctx, hipMemsetAsync(run.leaves_out, 0, leaf_b, ctx->stream));
    timing_begin(ctx);
    HIPCHECK(ctx, launch(ctx, 1, prog->d_desc, 1, run, prog->n_lds, ctx->stream));
    timing_end(ctx);
    HIPCHECK(ctx, hipMemcpyAsync(root_bits, run.root_bits, root_b, hipMemcpyDeviceToHost,
                                 ctx->stream));
    if (probe_b)
        HIPCHECK(ctx, hipMemcpyAsync(probes, run.probes, probe_b, hipMemcpyDeviceToHost,
                                     ctx->stream));
    if (leaf_b)
        HIPCHECK(ctx, hipMemcpyAsync(leaves_out, run.leaves_out, leaf_b, hipMemcpyDeviceToHost,
                                     ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    timing_read(ctx);
    return MG_OK;
}

// Candidates per launch of a search: launches are queued back to back with
// no host round trip; a wave whose candidates all lie beyond the program's
// current first witness exits at once (mg_run.skip_solved), so the search
// stops consuming lanes as soon as a witness is known.
#define MG_SEARCH_LAUNCH (1ull << 26)

int mg_search(mg_ctx* ctx, const mg_prog* prog, const mg_gen* gen, uint64_t n_cand,
              int64_t* first_sat, uint32_t* witness_leaves) {
    if (!ctx || !prog || !gen || !first_sat) return fail(ctx, MG_E_ARG, "null argument");
    *first_sat = -1;
    if (n_cand == 0) return MG_OK;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    const size_t leaf_b = (size_t)prog->n_leaves * 8 * 4;
    void* ws;
    int rc = workspace(ctx, 256 + leaf_b, &ws);
    if (rc) return rc;
    unsigned long long* d_first = (unsigned long long*)ws;
    HIPCHECK(ctx, hipMemsetAsync(d_first, 0xFF, 8, ctx->stream));
    timing_begin(ctx);
    for (uint64_t done = 0; done < n_cand; done += MG_SEARCH_LAUNCH) {
        mg_run run = empty_run();
        run.n_assign = n_cand - done < MG_SEARCH_LAUNCH ? n_cand - done : MG_SEARCH_LAUNCH;
        run.stride = run.n_assign;
        run.first_sat = d_first;
        run.seed = gen->seed;
        run.first_index = gen->first_index + done;
        run.skip_solved = 1;
        HIPCHECK(ctx, launch(ctx, 1, prog->d_desc, 1, run, prog->n_lds, ctx->stream));
    }
    timing_end(ctx);
    unsigned long long h = ~0ull;
    HIPCHECK(ctx, hipMemcpyAsync(&h, d_first, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    timing_read(ctx);
    if (h != ~0ull) *first_sat = (int64_t)h;
    if (*first_sat >= 0 && witness_leaves && prog->n_leaves) {
        // regenerate the winning candidate (counter-based streams: no gather)
        mg_run run = empty_run();
        run.n_assign = 1;
        run.stride = 1;
        run.seed = gen->seed;
        run.first_index = (uint64_t)*first_sat;
        run.leaves_out = (uint32_t*)((uint8_t*)ws + 256);
        HIPCHECK(ctx, hipMemsetAsync(run.leaves_out, 0, leaf_b, ctx->stream));
        HIPCHECK(ctx, launch(ctx, 1, prog->d_desc, 1, run, prog->n_lds, ctx->stream));
        HIPCHECK(ctx, hipMemcpyAsync(witness_leaves, run.leaves_out, leaf_b,
                                     hipMemcpyDeviceToHost, ctx->stream));
        HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MG_OK;
}

// What mg_census refuses for one program and its mask (mg_census_batch asks
// the same of every job): the message begins "census:".
static int census_check_job(mg_ctx* ctx, const mg_prog* prog, uint32_t n_roots,
                            uint32_t mask_probe0) {
    if (!mg_census_roots_ok(n_roots))
        return fail(ctx, MG_E_ARG, "census: n_roots %u outside 1..%u", n_roots, MG_CENSUS_MAX_ROOTS);
    if (!mg_census_mask_ok(prog->n_probes, n_roots, mask_probe0))
        return fail(ctx, MG_E_ARG, "census: mask probes %u..%u outside the program's %u probes",
                    mask_probe0, mask_probe0 + (n_roots + 255) / 256 - 1, prog->n_probes);
    return MG_OK;
}

// The arguments all programs of a census share; `who` begins the message
// ("census", "census_batch").
static int census_check_shared(mg_ctx* ctx, const char* who, const mg_gen* gen, uint64_t n_cand,
                               uint64_t chunk) {
    if (chunk % MG_BLOCK_LANES)
        return fail(ctx, MG_E_ARG, "%s: chunk %llu is not a multiple of %u", who,
                    (unsigned long long)chunk, MG_BLOCK_LANES);
    if (gen->first_index % 64)
        return fail(ctx, MG_E_ARG, "%s: first_index %llu is not a multiple of 64 (the "
                    "generator draws one class per 64 indices)", who,
                    (unsigned long long)gen->first_index);
    if (n_cand >= (1ull << MG_CENSUS_OFFSET_BITS) ||
        gen->first_index > (uint64_t)INT64_MAX - n_cand)
        return fail(ctx, MG_E_ARG, "%s: %llu candidates from %llu: at most 2^%d, indices "
                    "below 2^63", who, (unsigned long long)n_cand,
                    (unsigned long long)gen->first_index, MG_CENSUS_OFFSET_BITS);
    return MG_OK;
}

// The census of an empty range, and the outputs from a counter block h (as
// mg_census.h lays it out for n_roots) read back from the device.
static void census_empty(uint32_t n_roots, uint64_t* pass, uint64_t* first_block,
                         uint64_t* sole_block, int64_t* sole_index, uint64_t* nfail_hist,
                         uint32_t* best_nfail, int64_t* best_index) {
    for (uint32_t k = 0; k < n_roots; ++k) {
        pass[k] = first_block[k] = sole_block[k] = nfail_hist[k] = 0;
        sole_index[k] = -1;
    }
    nfail_hist[n_roots] = 0;
    *best_nfail = n_roots + 1;
    *best_index = -1;
}

static void census_unpack(const unsigned long long* h, uint32_t n_roots, uint64_t first_index,
                          uint64_t* pass, uint64_t* first_block, uint64_t* sole_block,
                          int64_t* sole_index, uint64_t* nfail_hist, uint32_t* best_nfail,
                          int64_t* best_index) {
    for (uint32_t k = 0; k < n_roots; ++k) {
        pass[k] = h[mg_census_pass(n_roots) + k];
        first_block[k] = h[mg_census_first(n_roots) + k];
        sole_block[k] = h[mg_census_sole(n_roots) + k];
        const unsigned long long si = h[mg_census_sole_index(n_roots) + k];
        sole_index[k] = si == ~0ull ? -1 : (int64_t)si;
    }
    for (uint32_t f = 0; f <= n_roots; ++f) nfail_hist[f] = h[mg_census_hist(n_roots) + f];
    const unsigned long long best = h[mg_census_best(n_roots)];
    if (best != ~0ull) {
        *best_nfail = (uint32_t)(best >> MG_CENSUS_OFFSET_BITS);
        *best_index = (int64_t)(first_index + (best & ((1ull << MG_CENSUS_OFFSET_BITS) - 1)));
    }
}

int mg_census(mg_ctx* ctx, const mg_prog* prog, const mg_gen* gen, uint64_t n_cand,
              uint32_t n_roots, uint32_t mask_probe0, uint64_t chunk, uint64_t* pass,
              uint64_t* first_block, uint64_t* sole_block, int64_t* sole_index,
              uint64_t* nfail_hist, uint32_t* best_nfail, int64_t* best_index) {
    if (!ctx || !prog || !gen || !pass || !first_block || !sole_block || !sole_index ||
        !nfail_hist || !best_nfail || !best_index)
        return fail(ctx, MG_E_ARG, "null argument");
    int rc = census_check_job(ctx, prog, n_roots, mask_probe0);
    if (rc == MG_OK) rc = census_check_shared(ctx, "census", gen, n_cand, chunk);
    if (rc != MG_OK) return rc;
    if (chunk == 0) chunk = MG_CENSUS_CHUNK;
    if (chunk > MG_CENSUS_MAX_PROBE_BYTES / 32 / prog->n_probes)
        return fail(ctx, MG_E_ARG, "census: %u probes x %llu candidates per chunk exceed a %zu MiB "
                    "probe buffer; load the census view of the program (census.census_view: "
                    "only the mask probes are written) or pass a smaller chunk", prog->n_probes,
                    (unsigned long long)chunk, MG_CENSUS_MAX_PROBE_BYTES >> 20);
    census_empty(n_roots, pass, first_block, sole_block, sole_index, nfail_hist, best_nfail,
                 best_index);
    if (n_cand == 0) return MG_OK;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    const uint64_t lanes = n_cand < chunk ? n_cand : chunk;       // of the largest launch
    const size_t count_b = ((size_t)mg_census_words(n_roots) * 8 + 255) & ~(size_t)255;
    const size_t probe_b = (size_t)prog->n_probes * 8 * lanes * 4;
    void* ws;
    rc = workspace(ctx, count_b + probe_b + 256, &ws);
    if (rc) return rc;
    unsigned long long* d_count = (unsigned long long*)ws;
    uint32_t* d_probes = (uint32_t*)((uint8_t*)ws + count_b);
    const size_t sums_b = (size_t)mg_census_sole_index(n_roots) * 8;
    HIPCHECK(ctx, hipMemsetAsync(d_count, 0, sums_b, ctx->stream));
    HIPCHECK(ctx, hipMemsetAsync((uint8_t*)d_count + sums_b, 0xFF,
                                 (size_t)mg_census_words(n_roots) * 8 - sums_b, ctx->stream));
    timing_begin(ctx);
    for (uint64_t done = 0; done < n_cand; done += chunk) {
        mg_run run = empty_run();
        run.n_assign = n_cand - done < chunk ? n_cand - done : chunk;
        run.stride = run.n_assign;
        run.probes = d_probes;
        run.seed = gen->seed;
        run.first_index = gen->first_index + done;
        HIPCHECK(ctx, launch(ctx, 1, prog->d_desc, 1, run, prog->n_lds, ctx->stream));
        HIPCHECK(ctx, mg_launch_census(d_probes + (size_t)mask_probe0 * 8 * run.stride, run.stride,
                                       run.n_assign, n_roots, run.first_index, done, d_count,
                                       ctx->stream));
    }
    timing_end(ctx);
    std::vector<unsigned long long> h(mg_census_words(n_roots));
    HIPCHECK(ctx, hipMemcpyAsync(h.data(), d_count, h.size() * 8, hipMemcpyDeviceToHost,
                                 ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    timing_read(ctx);
    census_unpack(h.data(), n_roots, gen->first_index, pass, first_block, sole_block, sole_index,
                  nfail_hist, best_nfail, best_index);
    return MG_OK;
}

// The censuses of several programs in one launch sequence (DESIGN.md §3.17,
// csrc/mg_census_batch.h, mg_census_batch.hip): mg_census with a job axis.
// Per chunk one interpreter launch over the batch's descriptor table, every
// job writing its own probe region (probes_per_prog), and one launch of the
// batched census kernel.  The row stride is the lanes of the largest launch
// in every chunk, the last one included, so a job's rows stay where its
// record says.
int mg_census_batch(mg_ctx* ctx, const mg_census_job* jobs, uint32_t n_jobs, const mg_gen* gen,
                    uint64_t n_cand, uint64_t chunk, uint32_t max_roots, uint64_t* pass,
                    uint64_t* first_block, uint64_t* sole_block, int64_t* sole_index,
                    uint64_t* nfail_hist, uint32_t* best_nfail, int64_t* best_index) {
    if (!ctx) return MG_E_ARG;
    if (!jobs || !gen || !pass || !first_block || !sole_block || !sole_index || !nfail_hist ||
        !best_nfail || !best_index)
        return fail(ctx, MG_E_ARG, "census_batch: null argument");
    if (n_jobs < 1 || n_jobs > MG_CENSUS_BATCH_MAX_JOBS)
        return fail(ctx, MG_E_ARG, "census_batch: %u jobs outside 1..%u", n_jobs,
                    MG_CENSUS_BATCH_MAX_JOBS);
    int rc = census_check_shared(ctx, "census_batch", gen, n_cand, chunk);
    if (rc != MG_OK) return rc;
    std::vector<mg_census_shape> shapes(n_jobs);
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_census_job& j = jobs[g];
        if (!j.prog) return fail(ctx, MG_E_ARG, "census_batch: job %u: null program", g);
        if (j.prog->ctx != ctx)
            return fail(ctx, MG_E_ARG, "census_batch: job %u: a program of another context", g);
        if (census_check_job(ctx, j.prog, j.n_roots, j.mask_probe0) != MG_OK) {
            const std::string why = ctx->err;
            return fail(ctx, MG_E_ARG, "census_batch: job %u: %s", g, why.c_str());
        }
        if (j.n_roots > max_roots)
            return fail(ctx, MG_E_ARG, "census_batch: job %u: n_roots %u above max_roots %u", g,
                        j.n_roots, max_roots);
        shapes[g] = {j.prog->n_probes, j.n_roots, j.mask_probe0};
    }
    std::vector<uint64_t> off(MG_CB_SHARED + (size_t)n_jobs * MG_CB_JOB_REGIONS);
    uint64_t bytes = 0, need = 0, count_w = 0, probe_w = 0, lanes_per = 0;
    const int st = mg_census_batch_plan(shapes.data(), n_jobs, n_cand, chunk, off.data(), &bytes,
                                        &lanes_per, &need, &count_w, &probe_w);
    if (st != MG_CB_OK) {
        char why[400];
        mg_census_batch_why(st, n_jobs, chunk, need, why, sizeof why);
        return fail(ctx, MG_E_ARG, "census_batch: %s", why);
    }
    chunk = lanes_per;
    const size_t hist = (size_t)max_roots + 1;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        // a row of max_roots entries per job: past the job's own roots, empty
        census_empty(max_roots, pass + (size_t)g * max_roots, first_block + (size_t)g * max_roots,
                     sole_block + (size_t)g * max_roots, sole_index + (size_t)g * max_roots,
                     nfail_hist + g * hist, best_nfail + g, best_index + g);
        best_nfail[g] = jobs[g].n_roots + 1;
    }
    if (n_cand == 0) return MG_OK;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    void* ws;
    rc = workspace(ctx, (size_t)bytes + 256, &ws);
    if (rc) return rc;
    uint8_t* w = (uint8_t*)ws;
    const uint64_t lanes = n_cand < chunk ? n_cand : chunk;       // of the largest launch
    // the host image of everything uploaded: descriptors, job records and the
    // counters (sums 0, minima ~0 per job), at the offsets of the plan
    const size_t up_b = (size_t)off[MG_CB_OFF(0, MG_CB_PROBES)];
    const size_t count0 = (size_t)off[MG_CB_OFF(0, MG_CB_COUNTS)];
    std::vector<uint8_t> img(up_b, 0);
    mg_pdesc* h_descs = (mg_pdesc*)(img.data() + off[MG_CB_DESCS]);
    mg_census_batch_job* h_jobs = (mg_census_batch_job*)(img.data() + off[MG_CB_JOBS]);
    uint32_t max_lds = 0;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_census_job& j = jobs[g];
        h_descs[g] = j.prog->h_desc;
        if (j.prog->n_lds > max_lds) max_lds = j.prog->n_lds;
        h_jobs[g].rows = (const uint32_t*)(w + off[MG_CB_OFF(g, MG_CB_PROBES)]) +
                         (size_t)j.mask_probe0 * 8 * lanes;
        h_jobs[g].out = (unsigned long long*)(w + off[MG_CB_OFF(g, MG_CB_COUNTS)]);
        h_jobs[g].n_roots = j.n_roots;
        unsigned long long* c = (unsigned long long*)(img.data() + off[MG_CB_OFF(g, MG_CB_COUNTS)]);
        for (uint32_t k = mg_census_sole_index(j.n_roots); k < mg_census_words(j.n_roots); ++k)
            c[k] = ~0ull;
    }
    HIPCHECK(ctx, hipMemcpyAsync(w, img.data(), up_b, hipMemcpyHostToDevice, ctx->stream));
    const mg_pdesc* d_descs = (const mg_pdesc*)(w + off[MG_CB_DESCS]);
    const mg_census_batch_job* d_jobs = (const mg_census_batch_job*)(w + off[MG_CB_JOBS]);
    timing_begin(ctx);
    for (uint64_t done = 0; done < n_cand; done += chunk) {
        mg_run run = empty_run();
        run.n_assign = n_cand - done < chunk ? n_cand - done : chunk;
        run.stride = lanes;
        run.probes = (uint32_t*)(w + off[MG_CB_OFF(0, MG_CB_PROBES)]);
        run.probes_per_prog = 1;
        run.probe_prog_words = probe_w;
        run.seed = gen->seed;
        run.first_index = gen->first_index + done;
        HIPCHECK(ctx, launch(ctx, 1, d_descs, n_jobs, run, max_lds, ctx->stream));
        HIPCHECK(ctx, mg_launch_census_batch(d_jobs, n_jobs, lanes, run.n_assign, run.first_index,
                                             done, ctx->stream));
    }
    timing_end(ctx);
    // all counter blocks in one copy (into the image's own counter regions)
    HIPCHECK(ctx, hipMemcpyAsync(img.data() + count0, w + count0, up_b - count0,
                                 hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    timing_read(ctx);
    for (uint32_t g = 0; g < n_jobs; ++g)
        census_unpack((const unsigned long long*)(img.data() + off[MG_CB_OFF(g, MG_CB_COUNTS)]),
                      jobs[g].n_roots, gen->first_index, pass + (size_t)g * max_roots,
                      first_block + (size_t)g * max_roots, sole_block + (size_t)g * max_roots,
                      sole_index + (size_t)g * max_roots, nfail_hist + g * hist, best_nfail + g,
                      best_index + g);
    return MG_OK;
}

int mg_census_batch_plan_host(const mg_census_shape* shapes, uint32_t n_jobs, uint64_t n_cand,
                              uint64_t chunk, uint64_t* out_offsets, uint64_t* out_bytes,
                              uint64_t* out_chunk, char* why, size_t why_len) {
    uint64_t need = 0;
    const int st = mg_census_batch_plan(shapes, n_jobs, n_cand, chunk, out_offsets, out_bytes,
                                        out_chunk, &need, nullptr, nullptr);
    mg_census_batch_why(st, n_jobs, chunk, need, why, why_len);
    return st == MG_CB_OK ? MG_OK : MG_E_ARG;
}

int mg_census_batch_blocks_host(uint32_t n_jobs, uint64_t n) {
    return (int)mg_census_batch_blocks(n_jobs, n);
}

// The local search.  Rounds are queued back to back; after
// every sync_every rounds the host reads the base's failing count (8 bytes)
// and stops at 0.
int mg_repair(mg_ctx* ctx, const mg_prog* prog, const uint32_t* start_leaves, uint32_t n_roots,
              uint32_t mask_probe0, uint64_t seed, uint32_t lanes, uint32_t max_rounds,
              uint32_t sync_every, uint32_t* out_leaves, uint32_t* out_nfail,
              uint32_t* out_rounds, uint32_t* trace) {
    if (!ctx || !prog || !start_leaves || !out_leaves || !out_nfail || !out_rounds)
        return fail(ctx, MG_E_ARG, "null argument");
    if (prog->n_leaves == 0) return fail(ctx, MG_E_ARG, "repair: the program has no leaves");
    if (n_roots < 1 || n_roots > MG_CENSUS_MAX_ROOTS)
        return fail(ctx, MG_E_ARG, "repair: n_roots %u outside 1..%u", n_roots, MG_CENSUS_MAX_ROOTS);
    const uint32_t n_mask = (n_roots + 255) / 256;
    if (mask_probe0 >= prog->n_probes || n_mask > prog->n_probes - mask_probe0)
        return fail(ctx, MG_E_ARG, "repair: mask probes %u..%u outside the program's %u probes",
                    mask_probe0, mask_probe0 + n_mask - 1, prog->n_probes);
    if (lanes < 1 || lanes > MG_REPAIR_MAX_LANES)
        return fail(ctx, MG_E_ARG, "repair: %u lanes outside 1..%u", lanes, MG_REPAIR_MAX_LANES);
    if (max_rounds < 1 || max_rounds > MG_REPAIR_MAX_ROUNDS)
        return fail(ctx, MG_E_ARG, "repair: %u rounds outside 1..%u", max_rounds,
                    MG_REPAIR_MAX_ROUNDS);
    if (lanes > MG_CENSUS_MAX_PROBE_BYTES / 32 / prog->n_probes)
        return fail(ctx, MG_E_ARG, "repair: %u probes x %u lanes exceed a %zu MiB probe buffer; "
                    "load the census view of the program (census.census_view: only the mask "
                    "probes are written) or pass fewer lanes", prog->n_probes, lanes,
                    MG_CENSUS_MAX_PROBE_BYTES >> 20);
    if (sync_every == 0) sync_every = 8;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const uint32_t n_leaves = prog->n_leaves;
    const uint64_t words = ((uint64_t)lanes + 63) / 64;
    const size_t base_b = (size_t)n_leaves * 32, gen_b = (size_t)n_leaves * sizeof(mg_leafgen),
                 trace_b = (size_t)max_rounds * 4, root_b = words * 8,
                 leaf_b = (size_t)n_leaves * 8 * lanes * 4,
                 probe_b = (size_t)prog->n_probes * 8 * lanes * 4;
    const size_t off_base = 256, off_gen = off_base + align(base_b),
                 off_trace = off_gen + align(gen_b), off_root = off_trace + align(trace_b),
                 off_leaf = off_root + align(root_b), off_probe = off_leaf + align(leaf_b),
                 total = off_probe + align(probe_b);
    void* ws;
    int rc = workspace(ctx, total + 256, &ws);
    if (rc) return rc;
    uint8_t* w = (uint8_t*)ws;
    mg_repair_state* d_state = (mg_repair_state*)w;
    uint32_t* d_base = (uint32_t*)(w + off_base);
    mg_leafgen* d_gen = (mg_leafgen*)(w + off_gen);
    uint32_t* d_trace = (uint32_t*)(w + off_trace);
    uint32_t* d_leaves = (uint32_t*)(w + off_leaf);
    uint32_t* d_probes = (uint32_t*)(w + off_probe);
    HIPCHECK(ctx, hipMemsetAsync(d_state, 0xFF, sizeof(mg_repair_state), ctx->stream));
    HIPCHECK(ctx, hipMemsetAsync(d_trace, 0, trace_b, ctx->stream));
    HIPCHECK(ctx, hipMemcpyAsync(d_base, start_leaves, base_b, hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(ctx, hipMemcpyAsync(d_gen, prog->leafgen.data(), gen_b, hipMemcpyHostToDevice,
                                 ctx->stream));
    mg_run run = empty_run();
    run.leaves = d_leaves;
    run.root_bits = (uint64_t*)(w + off_root);
    run.probes = d_probes;
    run.stride = lanes;
    run.n_assign = lanes;
    run.words_per_prog = words;
    const uint32_t* d_rows = d_probes + (size_t)mask_probe0 * 8 * lanes;
    const uint32_t* d_consts = prog->h_desc.consts;       // the first n_consts entries: as loaded
    uint32_t h_state[2] = {~0u, 0};                       // base_nfail, rounds
    timing_begin(ctx);
    uint32_t r = 0;
    while (r < max_rounds && h_state[0] != 0) {
        const uint32_t stop = max_rounds - r < sync_every ? max_rounds : r + sync_every;
        for (; r < stop; ++r) {
            HIPCHECK(ctx, mg_launch_repair_round(d_base, d_gen, d_consts, n_leaves, seed, r, lanes,
                                                 d_leaves, ctx->stream));
            HIPCHECK(ctx, launch(ctx, 0, prog->d_desc, 1, run, prog->n_lds, ctx->stream));
            HIPCHECK(ctx, mg_launch_repair_pick(d_rows, lanes, n_roots, d_base, d_gen, d_consts,
                                                n_leaves, seed, r, d_state, d_trace, ctx->stream));
        }
        timing_end(ctx);
        HIPCHECK(ctx, hipMemcpyAsync(h_state, &d_state->base_nfail, 8, hipMemcpyDeviceToHost,
                                     ctx->stream));
        HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    timing_read(ctx);
    HIPCHECK(ctx, hipMemcpyAsync(out_leaves, d_base, base_b, hipMemcpyDeviceToHost, ctx->stream));
    if (trace)
        HIPCHECK(ctx, hipMemcpyAsync(trace, d_trace, trace_b, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out_nfail = h_state[0];
    *out_rounds = r;
    return MG_OK;
}

// Host only: lanes lane0 .. lane0 + n_lanes - 1 of round r of the move
// function (mg_repair.h), as the mutate kernel writes them.
int mg_repair_mutate_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                          uint32_t n_consts, const uint32_t* base, uint64_t seed, uint32_t r,
                          uint32_t lanes, uint32_t lane0, uint32_t n_lanes, uint32_t* out,
                          uint32_t* moves) {
    if (!leaves || !base || !out || (n_consts && !consts) || n_leaves == 0) return MG_E_ARG;
    if (lanes < 1 || lanes > MG_REPAIR_MAX_LANES || r >= MG_REPAIR_MAX_ROUNDS) return MG_E_ARG;
    if (lane0 > lanes || n_lanes > lanes - lane0) return MG_E_ARG;
    for (uint32_t i = 0; i < n_leaves; ++i) {
        if (leaves[i].width < 1 || leaves[i].width > MG_MAX_WIDTH) return MG_E_ARG;
        if ((uint64_t)leaves[i].pool_off + leaves[i].pool_n > n_consts) return MG_E_ARG;
        uint32_t v[8];
        memcpy(v, base + (size_t)i * 8, 32);
        mg_repair_mask(v, leaves[i].width);
        if (memcmp(v, base + (size_t)i * 8, 32)) return MG_E_ARG;     // a base beyond its width
    }
    for (uint32_t a = 0; a < n_lanes; ++a) {
        mg_repair_moves mv;
        mg_repair_lane(base, leaves, consts, n_leaves, seed, r, lane0 + a, lanes, &mv);
        for (uint32_t leaf = 0; leaf < n_leaves; ++leaf) {
            uint32_t v[8];
            mg_repair_leaf(base, mv, mv.n, leaf, v);
            for (uint32_t k = 0; k < 8; ++k) out[((size_t)leaf * 8 + k) * n_lanes + a] = v[k];
        }
        if (moves) {
            moves[4 * (size_t)a] = mv.n;
            moves[4 * (size_t)a + 1] = mv.kind[0] | mv.kind[1] << 8;
            moves[4 * (size_t)a + 2] = mv.leaf[0];
            moves[4 * (size_t)a + 3] = mv.leaf[1];
        }
    }
    return MG_OK;
}

// a residual table entry names a known kind and, unless flat, a probe it has
static bool walk_table_ok(const uint32_t* table, uint32_t n_roots, uint32_t n_resid) {
    for (uint32_t k = 0; k < n_roots; ++k) {
        const uint32_t kind = table[k] >> 16, p = table[k] & 0xFFFFu;
        if (kind >= MG_WALK_KINDS || (kind != MG_WALK_FLAT && p >= n_resid)) return false;
    }
    return true;
}

// A walk is one mg_walk_job (include/mythgpu.h) and the rung of the ladder that
// runs it.  The rung says which of the job's tables are read, which checks and
// messages walk_check applies and which kernels walk_run launches; the fields
// a rung does not read are zero.  TABLE: roots is the residual table of
// mg_walk (no atoms, no code); TREE: the tree tables of mg_walk_tree; AIM: the
// round of mg_walk_aim with its aim table of 3-word entries; BOUND: the round
// of mg_walk_sum.hip, whose entries have 5 words and a fixed value each; UF:
// with the UF tables; SUM: with the lin words (below SUM: all 0) and n_srows
// side rows between the residual probes and the U rows.
enum walk_rung { TABLE, TREE, AIM, BOUND, UF, SUM };
static bool walk_tree(walk_rung g) { return g >= TREE; }
static bool walk_aim(walk_rung g) { return g >= AIM; }
static bool walk_bound(walk_rung g) { return g >= BOUND; }
static bool walk_uf(walk_rung g) { return g >= UF; }
static bool walk_sum(walk_rung g) { return g == SUM; }

// the job's UF tables (host pointers) as mg_walk_uf_ok and the kernels take them
static mg_uf_tables walk_uf_tables(const mg_walk_job& j) {
    return {j.slots, j.n_slots, j.funcs, j.n_funcs, j.cands, j.n_cands, j.ukeys, j.n_ukeys,
            j.n_urows};
}

// What every walk refuses before it uploads or launches anything (the
// message in ctx); mg_walk_batch asks the same of each of its jobs.
static int walk_check(mg_ctx* ctx, const mg_walk_job& j, walk_rung rung, uint32_t walkers,
                      uint32_t lanes, uint32_t max_rounds) {
    const mg_prog* prog = j.prog;
    const uint32_t* table = j.roots;
    const uint32_t n_roots = j.n_roots, mask_probe0 = j.mask_probe0, n_resid = j.n_resid;
    const mg_uf_tables uft = walk_uf_tables(j);
    if (!ctx || !prog || !j.starts || !table || !j.out_leaves || !j.out_nfail || !j.out_cost ||
        !j.out_rounds || !j.out_winner || (j.n_atoms && !j.atoms) || (j.n_code && !j.code) ||
        (j.n_entries && !j.entries) || (j.n_pieces && !j.pieces))
        return fail(ctx, MG_E_ARG, "null argument");
    if (walk_bound(rung) && j.n_entries && !j.fixed)
        return fail(ctx, MG_E_ARG, "walk_bound: null fixed values with %u entries", j.n_entries);
    if (prog->n_leaves == 0) return fail(ctx, MG_E_ARG, "walk: the program has no leaves");
    if (walkers < 1 || walkers > MG_WALK_MAX_WALKERS)
        return fail(ctx, MG_E_ARG, "walk: %u walkers outside 1..%u", walkers, MG_WALK_MAX_WALKERS);
    if (n_roots < 1 || n_roots > MG_CENSUS_MAX_ROOTS)
        return fail(ctx, MG_E_ARG, "walk: n_roots %u outside 1..%u", n_roots, MG_CENSUS_MAX_ROOTS);
    if (j.n_atoms > MG_WT_MAX_ATOMS)
        return fail(ctx, MG_E_ARG, "walk_tree: %u atoms (at most %u)", j.n_atoms,
                    MG_WT_MAX_ATOMS);
    // the root mask, then the atom mask (tree scoring), then the residuals
    const uint32_t n_mask = (n_roots + 255) / 256, n_amask = (j.n_atoms + 255) / 256;
    if (mask_probe0 >= prog->n_probes || n_mask > prog->n_probes - mask_probe0 ||
        n_amask > prog->n_probes - mask_probe0 - n_mask ||
        n_resid > prog->n_probes - mask_probe0 - n_mask - n_amask)
        return fail(ctx, MG_E_ARG, "walk: mask probes %u..%u and %u residual probes outside the "
                    "program's %u probes", mask_probe0, mask_probe0 + n_mask + n_amask - 1,
                    n_resid, prog->n_probes);
    if (lanes < 1 || lanes > MG_REPAIR_MAX_LANES)
        return fail(ctx, MG_E_ARG, "walk: %u lanes outside 1..%u", lanes, MG_REPAIR_MAX_LANES);
    if (max_rounds < 1 || max_rounds > MG_REPAIR_MAX_ROUNDS)
        return fail(ctx, MG_E_ARG, "walk: %u rounds outside 1..%u", max_rounds,
                    MG_REPAIR_MAX_ROUNDS);
    if (walk_tree(rung)) {
        if (!mg_walk_tree_ok(table, n_roots, j.atoms, j.n_atoms, j.code, j.n_code, n_resid))
            return fail(ctx, MG_E_ARG, "walk_tree: malformed tables (mg_walk_tree_ok: kinds, "
                        "atom and residual indices, offsets, stack depth, limits per root)");
    } else if (!walk_table_ok(table, n_roots, n_resid)) {
        return fail(ctx, MG_E_ARG, "walk: a table entry names an unknown kind or a residual "
                    "probe at or above %u", n_resid);
    }
    if (walk_sum(rung)) {
        const uint32_t room = prog->n_probes - mask_probe0 - n_mask - n_amask - n_resid;
        if (j.n_srows > MG_SUM_MAX_ROWS || j.n_srows > room || uft.n_urows > room - j.n_srows)
            return fail(ctx, MG_E_ARG, "walk_sum: %u side rows (at most %u) and %u U rows after "
                        "%u residual probes outside the program's %u probes", j.n_srows,
                        MG_SUM_MAX_ROWS, uft.n_urows, n_resid, prog->n_probes);
        if (j.n_entries && !j.lin)
            return fail(ctx, MG_E_ARG, "walk_sum: null lin words with %u entries", j.n_entries);
        if (!mg_walk_sum_ok(j.entries, j.n_entries, j.pieces, j.n_pieces, j.fixed, j.lin,
                            j.n_srows, prog->leafgen.data(), prog->n_leaves, n_resid, n_roots,
                            j.n_atoms, uft))
            return fail(ctx, MG_E_ARG, "walk_sum: malformed tables (mg_walk_sum_ok: what "
                        "mg_walk_uf_ok checks; an unknown lin word, the side row of a linear XOR "
                        "entry at or above %u, a side row in a linear order entry, a slot piece "
                        "in a linear entry, null tables)", j.n_srows);
    } else if (walk_uf(rung)) {
        if (uft.n_urows > prog->n_probes - mask_probe0 - n_mask - n_amask - n_resid)
            return fail(ctx, MG_E_ARG, "walk_uf: %u U rows after %u residual probes outside the "
                        "program's %u probes", uft.n_urows, n_resid, prog->n_probes);
        if (!mg_walk_uf_ok(j.entries, j.n_entries, j.pieces, j.n_pieces, j.fixed,
                           prog->leafgen.data(), prog->n_leaves, n_resid, n_roots, j.n_atoms,
                           uft))
            return fail(ctx, MG_E_ARG, "walk_uf: malformed tables (mg_walk_uf_ok: what "
                        "mg_walk_bound_ok checks for leaf pieces; at most %u slots, %u candidates "
                        "and %u U rows, null tables, slot, function, candidate, key and U-row "
                        "indices, 1..%u key chunks, one width per function's value leaves, a "
                        "slot piece outside it)", MG_UF_MAX_SLOTS, MG_UF_MAX_CANDS,
                        MG_UF_MAX_ROWS, MG_UF_MAX_CHUNKS);
    }
    if (rung == BOUND && !mg_walk_bound_ok(j.entries, j.n_entries, j.pieces, j.n_pieces, j.fixed,
                                           prog->leafgen.data(), prog->n_leaves, n_resid, n_roots,
                                           j.n_atoms))
        return fail(ctx, MG_E_ARG, "walk_bound: malformed aim table (mg_walk_bound_ok: what "
                    "mg_walk_aim_ok checks, a mode above %u, a truth index outside the %u atoms "
                    "or %u roots, an XOR entry with a truth or fixed word)", MG_BOUND_HIGH_STRICT,
                    j.n_atoms, n_roots);
    if (rung == AIM && !mg_walk_aim_ok(j.entries, j.n_entries, j.pieces, j.n_pieces,
                                       prog->leafgen.data(), prog->n_leaves, n_resid))
        return fail(ctx, MG_E_ARG, "walk_aim: malformed aim table (mg_walk_aim_ok: at most %u "
                    "entries of 1..%u pieces inside the piece array, residual and leaf indices, "
                    "bit ranges inside the leaf and the residual)", MG_AIM_MAX_ENTRIES,
                    MG_AIM_MAX_PIECES);
    const uint64_t total = (uint64_t)walkers * lanes;
    if (total > MG_CENSUS_MAX_PROBE_BYTES / 32 / prog->n_probes)
        return fail(ctx, MG_E_ARG, "walk: %u probes x %u walkers x %u lanes exceed a %zu MiB "
                    "probe buffer; load the census view of the program (census.census_view: "
                    "only the mask and residual probes are written) or pass fewer lanes",
                    prog->n_probes, walkers, lanes, MG_CENSUS_MAX_PROBE_BYTES >> 20);
    return MG_OK;
}

// One region of walk_run's workspace: filled from src when there is one, else
// with the byte fill (NO_FILL: left as it is); the pointer at dev, of whatever
// type, gets the region's device address.
struct walk_region {
    size_t bytes;
    const void* src;
    int fill;
    void* dev;
    size_t off;
};
enum { NO_FILL = -1 };

// The scored walk.  Rounds are queued back to back;
// after every sync_every rounds the host reads the walkers' states (16 bytes
// each) and stops once one of them has no failing root.
static int walk_run(mg_ctx* ctx, const mg_walk_job& j, walk_rung rung, uint32_t walkers,
                    uint32_t lanes, uint32_t max_rounds, uint32_t sync_every) {
    int ok = walk_check(ctx, j, rung, walkers, lanes, max_rounds);
    if (ok != MG_OK) return ok;
    const mg_prog* prog = j.prog;
    const uint32_t n_roots = j.n_roots, mask_probe0 = j.mask_probe0, n_resid = j.n_resid,
                   n_atoms = j.n_atoms, n_entries = j.n_entries, n_srows = j.n_srows;
    const uint64_t seed = j.seed;
    const bool tree = walk_tree(rung), aim = walk_aim(rung), bound = walk_bound(rung);
    const uint32_t n_mask = (n_roots + 255) / 256, n_amask = (n_atoms + 255) / 256;
    const uint64_t total = (uint64_t)walkers * lanes;
    if (sync_every == 0) sync_every = 8;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    const uint32_t n_leaves = prog->n_leaves;
    const uint64_t words = (total + 63) / 64;
    const size_t w32 = (size_t)walkers * 32, state_b = (size_t)walkers * sizeof(mg_walk_state),
                 base_b = w32 * n_leaves, trace_b = (size_t)walkers * max_rounds * 8;
    mg_walk_state* d_state;
    mg_leafgen* d_gen;
    uint64_t* d_root;
    uint32_t *d_bases, *d_table, *d_trace, *d_leaves, *d_probes, *d_atoms, *d_code, *d_entries,
             *d_pieces, *d_rstate, *d_lives, *d_fixed, *d_mstate, *d_ustate, *d_dests, *d_lin,
             *d_sstate;
    // the UF tables as the kernels read them: device pointers, host counts
    mg_uf_tables d_uf = walk_uf_tables(j);
    // The workspace in address order, every region 256-byte aligned.  The rung
    // decides the entry stride and which of the sum round's regions exist; a
    // rung below SUM has no lin words, so its lin region is zero: no entry is
    // linear.
    walk_region reg[] = {
        {state_b, nullptr, 0xFF, &d_state},
        {base_b, j.starts, NO_FILL, &d_bases},
        {(size_t)n_leaves * sizeof(mg_leafgen), prog->leafgen.data(), NO_FILL, &d_gen},
        {(size_t)n_roots * 4, j.roots, NO_FILL, &d_table},
        {trace_b, nullptr, 0, &d_trace},
        {words * 8, nullptr, NO_FILL, &d_root},
        {(size_t)n_leaves * 8 * total * 4, nullptr, NO_FILL, &d_leaves},
        {(size_t)prog->n_probes * 8 * total * 4, nullptr, NO_FILL, &d_probes},
        {(size_t)n_atoms * 4, j.atoms, NO_FILL, &d_atoms},
        {(size_t)j.n_code * 4, j.code, NO_FILL, &d_code},
        {(size_t)n_entries * (bound ? 20 : 12), j.entries, NO_FILL, &d_entries},
        {(size_t)j.n_pieces * 16, j.pieces, NO_FILL, &d_pieces},
        {aim ? w32 * n_resid : 0, nullptr, 0, &d_rstate},
        {aim ? (size_t)walkers * MG_AIM_LIVE_WORDS * 4 : 0, nullptr, 0, &d_lives},
        {bound ? (size_t)n_entries * 32 : 0, j.fixed, NO_FILL, &d_fixed},
        {bound ? (size_t)walkers * 4 * (MG_BOUND_MASK_WORDS(n_roots) +
                                        MG_BOUND_MASK_WORDS(n_atoms)) : 0, nullptr, 0, &d_mstate},
        {(size_t)j.n_slots * 8, j.slots, NO_FILL, &d_uf.slots},
        {(size_t)j.n_funcs * 12, j.funcs, NO_FILL, &d_uf.funcs},
        {(size_t)j.n_cands * 24, j.cands, NO_FILL, &d_uf.cands},
        {(size_t)j.n_ukeys * 32, j.ukeys, NO_FILL, &d_uf.ukeys},
        {w32 * j.n_urows, nullptr, 0, &d_ustate},
        {(size_t)walkers * j.n_slots * 4, nullptr, 0xFF, &d_dests},
        {bound ? (size_t)n_entries * 4 : 0, j.lin, 0, &d_lin},
        {w32 * n_srows, nullptr, 0, &d_sstate},
    };
    const size_t n_reg = sizeof reg / sizeof reg[0];
    size_t bytes = 0;
    for (walk_region& g : reg) {
        g.off = bytes;
        bytes += (g.bytes + 255) & ~(size_t)255;
    }
    void* ws;
    int rc = workspace(ctx, bytes + 256, &ws);
    if (rc) return rc;
    uint8_t* w = (uint8_t*)ws;
    // queued in address order, but for the trace's fill, which follows the state's
    static const uint8_t first[] = {0, 4, 1, 2, 3};
    for (size_t k = 0; k < n_reg; ++k) {
        const walk_region& g = reg[k < sizeof first ? first[k] : k];
        uint8_t* d = w + g.off;
        memcpy(g.dev, &d, sizeof d);
        if (g.bytes && g.src)
            HIPCHECK(ctx, hipMemcpyAsync(d, g.src, g.bytes, hipMemcpyHostToDevice, ctx->stream));
        else if (g.bytes && g.fill != NO_FILL)
            HIPCHECK(ctx, hipMemsetAsync(d, g.fill, g.bytes, ctx->stream));
    }
    mg_run run = empty_run();
    run.leaves = d_leaves;
    run.root_bits = d_root;
    run.probes = d_probes;
    run.stride = total;
    run.n_assign = total;
    run.words_per_prog = words;
    const uint32_t* d_masks = d_probes + (size_t)mask_probe0 * 8 * total;
    const uint32_t* d_amasks = d_masks + (size_t)n_mask * 8 * total;
    const uint32_t* d_resid = d_amasks + (size_t)n_amask * 8 * total;
    const uint32_t* d_srows = d_resid + (size_t)n_resid * 8 * total;
    const uint32_t* d_urows = d_srows + (size_t)n_srows * 8 * total;
    const uint32_t* d_consts = prog->h_desc.consts;       // the first n_consts entries: as loaded
    std::vector<mg_walk_state> h_state(walkers);
    bool done = false;
    timing_begin(ctx);
    uint32_t r = 0;
    while (r < max_rounds && !done) {
        const uint32_t stop = max_rounds - r < sync_every ? max_rounds : r + sync_every;
        for (; r < stop; ++r) {
            if (bound)                      // mg_walk_bound, mg_walk_uf, mg_walk_sum
                HIPCHECK(ctx, mg_launch_walk_sum_round(d_bases, d_gen, d_consts, n_leaves, seed,
                                                       r, lanes, walkers, d_entries, n_entries,
                                                       d_pieces, d_fixed, d_lin, d_rstate, n_resid,
                                                       d_sstate, n_srows, d_lives, d_dests,
                                                       d_uf.n_slots, d_leaves, ctx->stream));
            else if (aim)
                HIPCHECK(ctx, mg_launch_walk_aim_round(d_bases, d_gen, d_consts, n_leaves, seed, r,
                                                       lanes, walkers, d_entries, n_entries,
                                                       d_pieces, d_rstate, n_resid, d_lives,
                                                       d_leaves, ctx->stream));
            else
                HIPCHECK(ctx, mg_launch_walk_round(d_bases, d_gen, d_consts, n_leaves, seed, r,
                                                   lanes, walkers, d_leaves, ctx->stream));
            HIPCHECK(ctx, launch(ctx, 0, prog->d_desc, 1, run, prog->n_lds, ctx->stream));
            if (bound)
                HIPCHECK(ctx, mg_launch_walk_sum_pick(d_masks, d_amasks, d_resid, d_srows, n_srows,
                                                      d_urows, d_table, d_atoms, d_code, lanes,
                                                      walkers, n_roots, n_atoms, d_bases, d_gen,
                                                      d_consts, n_leaves, seed, r, max_rounds,
                                                      d_entries, n_entries, d_pieces, d_fixed,
                                                      d_lin, n_resid, d_uf, d_rstate, d_mstate,
                                                      d_sstate, d_ustate, d_dests, d_lives,
                                                      d_state, d_trace, ctx->stream));
            else if (aim)
                HIPCHECK(ctx, mg_launch_walk_aim_pick(d_masks, d_amasks, d_resid, d_table, d_atoms,
                                                      d_code, lanes, walkers, n_roots, d_bases,
                                                      d_gen, d_consts, n_leaves, seed, r,
                                                      max_rounds, d_entries, n_entries,
                                                      d_pieces, n_resid, d_rstate, d_lives,
                                                      d_state, d_trace, ctx->stream));
            else if (tree)
                HIPCHECK(ctx, mg_launch_walk_tree_pick(d_masks, d_amasks, d_resid, d_table,
                                                       d_atoms, d_code, lanes, walkers, n_roots,
                                                       d_bases, d_gen, d_consts, n_leaves, seed,
                                                       r, max_rounds, d_state, d_trace,
                                                       ctx->stream));
            else
                HIPCHECK(ctx, mg_launch_walk_pick(d_masks, d_resid, d_table, lanes, walkers,
                                                  n_roots, d_bases, d_gen, d_consts, n_leaves,
                                                  seed, r, max_rounds, d_state, d_trace,
                                                  ctx->stream));
        }
        timing_end(ctx);
        HIPCHECK(ctx, hipMemcpyAsync(h_state.data(), d_state, state_b, hipMemcpyDeviceToHost,
                                     ctx->stream));
        HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t k = 0; k < walkers; ++k) done = done || h_state[k].nfail == 0;
    }
    timing_read(ctx);
    HIPCHECK(ctx, hipMemcpyAsync(j.out_leaves, d_bases, base_b, hipMemcpyDeviceToHost, ctx->stream));
    if (j.trace)
        HIPCHECK(ctx, hipMemcpyAsync(j.trace, d_trace, trace_b, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t win = 0;
    for (uint32_t k = 0; k < walkers; ++k) {
        j.out_nfail[k] = h_state[k].nfail;
        j.out_cost[k] = h_state[k].cost;
        if (h_state[k].nfail < h_state[win].nfail ||
            (h_state[k].nfail == h_state[win].nfail && h_state[k].cost < h_state[win].cost))
            win = k;
    }
    *j.out_rounds = r;
    *j.out_winner = win;
    return MG_OK;
}

// A zeroed job j with the fields that every walk entry takes, under the job's
// own names; the entry adds its rung's tables.
#define WALK_JOB(j)                                                                         \
    mg_walk_job j = {};                                                                     \
    j.prog = prog, j.starts = starts, j.n_roots = n_roots, j.mask_probe0 = mask_probe0;     \
    j.n_resid = n_resid, j.seed = seed, j.out_leaves = out_leaves, j.out_nfail = out_nfail; \
    j.out_cost = out_cost, j.out_rounds = out_rounds, j.trace = trace, j.out_winner = out_winner

int mg_walk(mg_ctx* ctx, const mg_prog* prog, const uint32_t* starts, uint32_t walkers,
            uint32_t n_roots, uint32_t mask_probe0, const uint32_t* table, uint32_t n_resid,
            uint64_t seed, uint32_t lanes, uint32_t max_rounds, uint32_t sync_every,
            uint32_t* out_leaves, uint32_t* out_nfail, uint32_t* out_cost, uint32_t* out_rounds,
            uint32_t* trace, uint32_t* out_winner) {
    WALK_JOB(j);
    j.roots = table;
    return walk_run(ctx, j, TABLE, walkers, lanes, max_rounds, sync_every);
}

// The scored walk with tree distances: mg_walk with the
// tables of mg_walk_tree.h in place of the residual table.
int mg_walk_tree(mg_ctx* ctx, const mg_prog* prog, const uint32_t* starts, uint32_t walkers,
                 uint32_t n_roots, uint32_t mask_probe0, const uint32_t* roots, uint32_t n_atoms,
                 const uint32_t* atoms, const uint32_t* code, uint32_t n_code, uint32_t n_resid,
                 uint64_t seed, uint32_t lanes, uint32_t max_rounds, uint32_t sync_every,
                 uint32_t* out_leaves, uint32_t* out_nfail, uint32_t* out_cost,
                 uint32_t* out_rounds, uint32_t* trace, uint32_t* out_winner) {
    WALK_JOB(j);
    j.roots = roots, j.atoms = atoms, j.n_atoms = n_atoms, j.code = code, j.n_code = n_code;
    return walk_run(ctx, j, TREE, walkers, lanes, max_rounds, sync_every);
}

// The tree-scored walk with aimed moves: mg_walk_tree with
// the mutate and adopt kernels of mg_walk_aim.hip and their aim table.
int mg_walk_aim(mg_ctx* ctx, const mg_prog* prog, const uint32_t* starts, uint32_t walkers,
                uint32_t n_roots, uint32_t mask_probe0, const uint32_t* roots, uint32_t n_atoms,
                const uint32_t* atoms, const uint32_t* code, uint32_t n_code, uint32_t n_resid,
                const uint32_t* entries, uint32_t n_entries, const uint32_t* pieces,
                uint32_t n_pieces, uint64_t seed, uint32_t lanes, uint32_t max_rounds,
                uint32_t sync_every, uint32_t* out_leaves, uint32_t* out_nfail,
                uint32_t* out_cost, uint32_t* out_rounds, uint32_t* trace, uint32_t* out_winner) {
    WALK_JOB(j);
    j.roots = roots, j.atoms = atoms, j.n_atoms = n_atoms, j.code = code, j.n_code = n_code;
    j.entries = entries, j.n_entries = n_entries, j.pieces = pieces, j.n_pieces = n_pieces;
    return walk_run(ctx, j, AIM, walkers, lanes, max_rounds, sync_every);
}

// The tree-scored walk with moves aimed by equalities and orders (DESIGN.md
// §3.13): mg_walk_aim with the kernels of mg_walk_sum.hip and the 5-word table
// of mg_walk_bound.h (no UF table, no lin word).
int mg_walk_bound(mg_ctx* ctx, const mg_prog* prog, const uint32_t* starts, uint32_t walkers,
                  uint32_t n_roots, uint32_t mask_probe0, const uint32_t* roots, uint32_t n_atoms,
                  const uint32_t* atoms, const uint32_t* code, uint32_t n_code, uint32_t n_resid,
                  const uint32_t* entries, uint32_t n_entries, const uint32_t* pieces,
                  uint32_t n_pieces, const uint32_t* fixed, uint64_t seed, uint32_t lanes,
                  uint32_t max_rounds, uint32_t sync_every, uint32_t* out_leaves,
                  uint32_t* out_nfail, uint32_t* out_cost, uint32_t* out_rounds, uint32_t* trace,
                  uint32_t* out_winner) {
    WALK_JOB(j);
    j.roots = roots, j.atoms = atoms, j.n_atoms = n_atoms, j.code = code, j.n_code = n_code;
    j.entries = entries, j.n_entries = n_entries, j.pieces = pieces, j.n_pieces = n_pieces;
    j.fixed = fixed;
    return walk_run(ctx, j, BOUND, walkers, lanes, max_rounds, sync_every);
}

// The same with aims that write the table entry a UF application reads
// (DESIGN.md §3.14): mg_walk_bound with the UF tables of mg_walk_uf.h and
// n_urows U rows after the residual probes.
int mg_walk_uf(mg_ctx* ctx, const mg_prog* prog, const uint32_t* starts, uint32_t walkers,
               uint32_t n_roots, uint32_t mask_probe0, const uint32_t* roots, uint32_t n_atoms,
               const uint32_t* atoms, const uint32_t* code, uint32_t n_code, uint32_t n_resid,
               const uint32_t* entries, uint32_t n_entries, const uint32_t* pieces,
               uint32_t n_pieces, const uint32_t* fixed, const uint32_t* slots, uint32_t n_slots,
               const uint32_t* funcs, uint32_t n_funcs, const uint32_t* cands, uint32_t n_cands,
               const uint32_t* ukeys, uint32_t n_ukeys, uint32_t n_urows, uint64_t seed,
               uint32_t lanes, uint32_t max_rounds, uint32_t sync_every, uint32_t* out_leaves,
               uint32_t* out_nfail, uint32_t* out_cost, uint32_t* out_rounds, uint32_t* trace,
               uint32_t* out_winner) {
    if (ctx) HIPCHECK(ctx, hipSetDevice(ctx->device));
    WALK_JOB(j);
    j.roots = roots, j.atoms = atoms, j.n_atoms = n_atoms, j.code = code, j.n_code = n_code;
    j.entries = entries, j.n_entries = n_entries, j.pieces = pieces, j.n_pieces = n_pieces;
    j.fixed = fixed, j.n_urows = n_urows;
    j.slots = slots, j.n_slots = n_slots, j.funcs = funcs, j.n_funcs = n_funcs;
    j.cands = cands, j.n_cands = n_cands, j.ukeys = ukeys, j.n_ukeys = n_ukeys;
    return walk_run(ctx, j, UF, walkers, lanes, max_rounds, sync_every);
}

// The same with aims through sums, differences, masks and shifts (DESIGN.md
// §3.15): mg_walk_uf with the lin words of mg_walk_sum.h and n_srows side rows
// between the residual probes and the U rows.
int mg_walk_sum(mg_ctx* ctx, const mg_prog* prog, const uint32_t* starts, uint32_t walkers,
                uint32_t n_roots, uint32_t mask_probe0, const uint32_t* roots, uint32_t n_atoms,
                const uint32_t* atoms, const uint32_t* code, uint32_t n_code, uint32_t n_resid,
                const uint32_t* entries, uint32_t n_entries, const uint32_t* pieces,
                uint32_t n_pieces, const uint32_t* fixed, const uint32_t* lin, uint32_t n_srows,
                const uint32_t* slots, uint32_t n_slots, const uint32_t* funcs, uint32_t n_funcs,
                const uint32_t* cands, uint32_t n_cands, const uint32_t* ukeys, uint32_t n_ukeys,
                uint32_t n_urows, uint64_t seed, uint32_t lanes, uint32_t max_rounds,
                uint32_t sync_every, uint32_t* out_leaves, uint32_t* out_nfail,
                uint32_t* out_cost, uint32_t* out_rounds, uint32_t* trace, uint32_t* out_winner) {
    if (ctx) HIPCHECK(ctx, hipSetDevice(ctx->device));
    WALK_JOB(j);
    j.roots = roots, j.atoms = atoms, j.n_atoms = n_atoms, j.code = code, j.n_code = n_code;
    j.entries = entries, j.n_entries = n_entries, j.pieces = pieces, j.n_pieces = n_pieces;
    j.fixed = fixed, j.lin = lin, j.n_srows = n_srows, j.n_urows = n_urows;
    j.slots = slots, j.n_slots = n_slots, j.funcs = funcs, j.n_funcs = n_funcs;
    j.cands = cands, j.n_cands = n_cands, j.ukeys = ukeys, j.n_ukeys = n_ukeys;
    return walk_run(ctx, j, SUM, walkers, lanes, max_rounds, sync_every);
}

// The walks of several groups in one launch sequence (DESIGN.md §3.16,
// csrc/mg_walk_batch.h, mg_walk_batch.hip): the round of mg_walk_sum with a
// job axis, every job stopped at the sync point where its own walk stops.
static mg_walk_shape walk_job_shape(const mg_walk_job& j) {
    mg_walk_shape s;
    s.n_leaves = j.prog->n_leaves;
    s.n_probes = j.prog->n_probes;
    s.n_roots = j.n_roots;
    s.mask_probe0 = j.mask_probe0;
    s.n_atoms = j.n_atoms;
    s.n_code = j.n_code;
    s.n_resid = j.n_resid;
    s.n_entries = j.n_entries;
    s.n_pieces = j.n_pieces;
    s.n_srows = j.n_srows;
    s.n_slots = j.n_slots;
    s.n_funcs = j.n_funcs;
    s.n_cands = j.n_cands;
    s.n_ukeys = j.n_ukeys;
    s.n_urows = j.n_urows;
    return s;
}

int mg_walk_batch(mg_ctx* ctx, const mg_walk_job* jobs, uint32_t n_jobs, uint32_t walkers,
                  uint32_t lanes, uint32_t max_rounds, uint32_t sync_every, uint64_t max_bytes) {
    if (!ctx) return MG_E_ARG;
    if (n_jobs < 1 || n_jobs > MG_WALK_BATCH_MAX_JOBS)
        return fail(ctx, MG_E_ARG, "walk_batch: %u jobs outside 1..%u", n_jobs,
                    MG_WALK_BATCH_MAX_JOBS);
    if (walkers < 1 || walkers > MG_WALK_MAX_WALKERS)
        return fail(ctx, MG_E_ARG, "walk_batch: %u walkers outside 1..%u", walkers,
                    MG_WALK_MAX_WALKERS);
    if (lanes < 1 || lanes > MG_REPAIR_MAX_LANES)
        return fail(ctx, MG_E_ARG, "walk_batch: %u lanes outside 1..%u", lanes,
                    MG_REPAIR_MAX_LANES);
    if (max_rounds < 1 || max_rounds > MG_REPAIR_MAX_ROUNDS)
        return fail(ctx, MG_E_ARG, "walk_batch: %u rounds outside 1..%u", max_rounds,
                    MG_REPAIR_MAX_ROUNDS);
    if (!jobs) return fail(ctx, MG_E_ARG, "walk_batch: null jobs");
    std::vector<mg_walk_shape> shapes(n_jobs);
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_walk_job& j = jobs[g];
        if (!j.prog || !j.starts || !j.roots || !j.out_leaves || !j.out_nfail || !j.out_cost ||
            !j.out_rounds || !j.out_winner)
            return fail(ctx, MG_E_ARG, "walk_batch: job %u: null program, starts, roots or "
                        "output pointer", g);
        if (j.prog->ctx != ctx)
            return fail(ctx, MG_E_ARG, "walk_batch: job %u: a program of another context", g);
        if (walk_check(ctx, j, SUM, walkers, lanes, max_rounds) != MG_OK) {
            const std::string why = ctx->err;
            return fail(ctx, MG_E_ARG, "walk_batch: job %u: %s", g, why.c_str());
        }
        shapes[g] = walk_job_shape(j);
        if (!mg_walk_batch_shape_ok(shapes[g]))        // implied by the checks above
            return fail(ctx, MG_E_ARG, "walk_batch: job %u: counts out of range", g);
    }
    std::vector<uint64_t> off(MG_WB_SHARED + (size_t)n_jobs * MG_WB_JOB_REGIONS);
    uint64_t bytes = 0, leaf_w = 0, probe_w = 0;
    if (!mg_walk_batch_plan(shapes.data(), n_jobs, walkers, lanes, max_rounds, off.data(), &bytes,
                            &leaf_w, &probe_w))
        return fail(ctx, MG_E_ARG, "walk_batch: the batch's buffer exceeds 64 bits");
    if (max_bytes == 0) max_bytes = MG_WALK_BATCH_DEFAULT_BYTES;
    if (bytes > max_bytes)
        return fail(ctx, MG_E_ARG, "walk_batch: %llu bytes needed for %u jobs, max_bytes is %llu",
                    (unsigned long long)bytes, n_jobs, (unsigned long long)max_bytes);
    if (sync_every == 0) sync_every = 8;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    void* ws;
    int rc = workspace(ctx, (size_t)bytes + 256, &ws);
    if (rc) return rc;
    uint8_t* w = (uint8_t*)ws;
    const uint64_t total = (uint64_t)walkers * lanes, words = (total + 63) / 64;
    // the host image of everything uploaded: descriptors, jobs, frozen words
    // (zero) and every job's tables, at the offsets of the plan
    const size_t up_b = (size_t)off[MG_WB_OFF(0, MG_WB_FIRST_ZEROED)];
    const size_t zero_b = (size_t)(off[MG_WB_STATES] - up_b);
    const size_t ones_b = (size_t)(off[MG_WB_ROOTBITS] - off[MG_WB_STATES]);
    std::vector<uint8_t> img(up_b, 0);
    mg_pdesc* h_descs = (mg_pdesc*)(img.data() + off[MG_WB_DESCS]);
    mg_walk_batch_job* h_jobs = (mg_walk_batch_job*)(img.data() + off[MG_WB_JOBS]);
    mg_walk_state* d_states = (mg_walk_state*)(w + off[MG_WB_STATES]);
    uint32_t max_lds = 0;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_walk_job& j = jobs[g];
        const mg_walk_shape& s = shapes[g];
        auto at = [&](uint32_t k) { return off[MG_WB_OFF(g, k)]; };
        auto put = [&](uint32_t k, const void* src, size_t n) {
            if (n) memcpy(img.data() + at(k), src, n);
        };
        put(MG_WB_BASES, j.starts, (size_t)walkers * s.n_leaves * 32);
        put(MG_WB_GEN, j.prog->leafgen.data(), (size_t)s.n_leaves * sizeof(mg_leafgen));
        put(MG_WB_ROOTS, j.roots, (size_t)s.n_roots * 4);
        put(MG_WB_ATOMS, j.atoms, (size_t)s.n_atoms * 4);
        put(MG_WB_CODE, j.code, (size_t)s.n_code * 4);
        put(MG_WB_ENTRIES, j.entries, (size_t)s.n_entries * 20);
        put(MG_WB_PIECES, j.pieces, (size_t)s.n_pieces * 16);
        put(MG_WB_FIXED, j.fixed, (size_t)s.n_entries * 32);
        put(MG_WB_LIN, j.lin, (size_t)s.n_entries * 4);
        put(MG_WB_SLOTS, j.slots, (size_t)s.n_slots * 8);
        put(MG_WB_FUNCS, j.funcs, (size_t)s.n_funcs * 12);
        put(MG_WB_CANDS, j.cands, (size_t)s.n_cands * 24);
        put(MG_WB_UKEYS, j.ukeys, (size_t)s.n_ukeys * 32);
        h_descs[g] = j.prog->h_desc;
        if (j.prog->n_lds > max_lds) max_lds = j.prog->n_lds;
        const uint32_t n_mask = (s.n_roots + 255) / 256, n_amask = (s.n_atoms + 255) / 256;
        mg_walk_batch_job& d = h_jobs[g];
        d.bases = (uint32_t*)(w + at(MG_WB_BASES));
        d.gen = (const mg_leafgen*)(w + at(MG_WB_GEN));
        d.consts = j.prog->h_desc.consts;             // the first n_consts entries: as loaded
        d.roots = (const uint32_t*)(w + at(MG_WB_ROOTS));
        d.atoms = (const uint32_t*)(w + at(MG_WB_ATOMS));
        d.code = (const uint32_t*)(w + at(MG_WB_CODE));
        d.entries = (const uint32_t*)(w + at(MG_WB_ENTRIES));
        d.pieces = (const uint32_t*)(w + at(MG_WB_PIECES));
        d.fixed = (const uint32_t*)(w + at(MG_WB_FIXED));
        d.lin = (const uint32_t*)(w + at(MG_WB_LIN));
        d.slots = (const uint32_t*)(w + at(MG_WB_SLOTS));
        d.funcs = (const uint32_t*)(w + at(MG_WB_FUNCS));
        d.cands = (const uint32_t*)(w + at(MG_WB_CANDS));
        d.ukeys = (const uint32_t*)(w + at(MG_WB_UKEYS));
        d.rstate = (uint32_t*)(w + at(MG_WB_RSTATE));
        d.mstate = (uint32_t*)(w + at(MG_WB_MSTATE));
        d.sstate = (uint32_t*)(w + at(MG_WB_SSTATE));
        d.ustate = (uint32_t*)(w + at(MG_WB_USTATE));
        d.dests = (uint32_t*)(w + at(MG_WB_DESTS));
        d.lives = (uint32_t*)(w + at(MG_WB_LIVES));
        d.state = d_states + (size_t)g * walkers;
        d.trace = (uint32_t*)(w + at(MG_WB_TRACE));
        d.leaves = (uint32_t*)(w + at(MG_WB_LEAVES));
        // in the job's probe region: as mg_walk_sum lays its probes out
        d.masks = (const uint32_t*)(w + at(MG_WB_PROBES)) + (size_t)s.mask_probe0 * 8 * total;
        d.amasks = d.masks + (size_t)n_mask * 8 * total;
        d.resid = d.amasks + (size_t)n_amask * 8 * total;
        d.srows = d.resid + (size_t)s.n_resid * 8 * total;
        d.urows = d.srows + (size_t)s.n_srows * 8 * total;
        d.seed = j.seed;
        d.n_leaves = s.n_leaves;
        d.n_roots = s.n_roots;
        d.n_atoms = s.n_atoms;
        d.n_resid = s.n_resid;
        d.n_entries = s.n_entries;
        d.n_srows = s.n_srows;
        d.n_urows = s.n_urows;
        d.n_slots = s.n_slots;
    }
    const mg_pdesc* d_descs = (const mg_pdesc*)(w + off[MG_WB_DESCS]);
    const mg_walk_batch_job* d_jobs = (const mg_walk_batch_job*)(w + off[MG_WB_JOBS]);
    uint32_t* d_frozen = (uint32_t*)(w + off[MG_WB_FROZEN]);
    HIPCHECK(ctx, hipMemcpyAsync(w, img.data(), up_b, hipMemcpyHostToDevice, ctx->stream));
    if (zero_b) HIPCHECK(ctx, hipMemsetAsync(w + up_b, 0, zero_b, ctx->stream));
    HIPCHECK(ctx, hipMemsetAsync(d_states, 0xFF, ones_b, ctx->stream));
    mg_run run = empty_run();
    run.leaves = (const uint32_t*)(w + off[MG_WB_OFF(0, MG_WB_LEAVES)]);
    run.leaves_prog_words = leaf_w;
    run.probes = (uint32_t*)(w + off[MG_WB_OFF(0, MG_WB_PROBES)]);
    run.probe_prog_words = probe_w;
    run.probes_per_prog = 1;
    run.skip_prog = d_frozen;
    run.root_bits = (uint64_t*)(w + off[MG_WB_ROOTBITS]);
    run.stride = total;
    run.n_assign = total;
    run.words_per_prog = words;
    const size_t state_b = (size_t)n_jobs * walkers * sizeof(mg_walk_state);
    std::vector<mg_walk_state> h_state((size_t)n_jobs * walkers);
    std::vector<uint32_t> h_frozen(n_jobs, 0), rounds(n_jobs, max_rounds);
    uint32_t live = n_jobs;
    timing_begin(ctx);
    uint32_t r = 0;
    while (r < max_rounds && live) {
        const uint32_t stop = max_rounds - r < sync_every ? max_rounds : r + sync_every;
        for (; r < stop; ++r) {
            HIPCHECK(ctx, mg_launch_walk_batch_round(d_jobs, d_frozen, n_jobs, r, lanes, walkers,
                                                     max_rounds, ctx->stream));
            HIPCHECK(ctx, launch(ctx, 0, d_descs, n_jobs, run, max_lds, ctx->stream));
            HIPCHECK(ctx, mg_launch_walk_batch_pick(d_jobs, d_frozen, n_jobs, r, lanes, walkers,
                                                    max_rounds, ctx->stream));
        }
        timing_end(ctx);
        HIPCHECK(ctx, hipMemcpyAsync(h_state.data(), d_states, state_b, hipMemcpyDeviceToHost,
                                     ctx->stream));
        HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
        bool froze = false;
        for (uint32_t g = 0; g < n_jobs; ++g) {
            if (h_frozen[g]) continue;
            bool done = false;
            for (uint32_t k = 0; k < walkers; ++k)
                done = done || h_state[(size_t)g * walkers + k].nfail == 0;
            if (!done) continue;
            h_frozen[g] = 1;                   // where the single walk of g stops
            rounds[g] = r;
            --live;
            froze = true;
        }
        if (froze && live && r < max_rounds)
            HIPCHECK(ctx, hipMemcpyAsync(d_frozen, h_frozen.data(), (size_t)n_jobs * 4,
                                         hipMemcpyHostToDevice, ctx->stream));
    }
    timing_read(ctx);
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_walk_job& j = jobs[g];
        HIPCHECK(ctx, hipMemcpyAsync(j.out_leaves, w + off[MG_WB_OFF(g, MG_WB_BASES)],
                                     (size_t)walkers * shapes[g].n_leaves * 32,
                                     hipMemcpyDeviceToHost, ctx->stream));
        if (j.trace)
            HIPCHECK(ctx, hipMemcpyAsync(j.trace, w + off[MG_WB_OFF(g, MG_WB_TRACE)],
                                         (size_t)walkers * max_rounds * 8, hipMemcpyDeviceToHost,
                                         ctx->stream));
    }
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_walk_job& j = jobs[g];
        const mg_walk_state* st = h_state.data() + (size_t)g * walkers;
        uint32_t win = 0;
        for (uint32_t k = 0; k < walkers; ++k) {
            j.out_nfail[k] = st[k].nfail;
            j.out_cost[k] = st[k].cost;
            if (st[k].nfail < st[win].nfail ||
                (st[k].nfail == st[win].nfail && st[k].cost < st[win].cost))
                win = k;
        }
        *j.out_rounds = rounds[g] < r ? rounds[g] : r;
        *j.out_winner = win;
    }
    return MG_OK;
}

int mg_walk_batch_plan_host(const mg_walk_shape* shapes, uint32_t n_jobs, uint32_t walkers,
                            uint32_t lanes, uint32_t max_rounds, uint64_t* out_offsets,
                            uint64_t* out_bytes) {
    return mg_walk_batch_plan(shapes, n_jobs, walkers, lanes, max_rounds, out_offsets, out_bytes,
                              nullptr, nullptr) ? MG_OK : MG_E_ARG;
}

int mg_walk_batch_shape_ok_host(const mg_walk_shape* shape) {
    return shape && mg_walk_batch_shape_ok(*shape) ? 1 : 0;
}

// Witness carry (include/mythgpu.h mg_carry_batch, DESIGN.md §3.18;
// csrc/mg_carry.h, mg_carry.hip): fill, one eval-mode launch over the job
// axis, gather; one upload before and one download after.
int mg_carry_batch(mg_ctx* ctx, const mg_carry_job* jobs, uint32_t n_jobs, const mg_gen* gen,
                   uint32_t lanes, int64_t* first, uint32_t* leaves, uint32_t max_leaves,
                   uint32_t* fill_out) {
    if (!ctx) return MG_E_ARG;
    if (!jobs || !gen || !first || !leaves)
        return fail(ctx, MG_E_ARG, "carry_batch: null argument");
    if (n_jobs < 1 || n_jobs > MG_CARRY_MAX_JOBS)
        return fail(ctx, MG_E_ARG, "carry_batch: %u jobs outside 1..%u", n_jobs,
                    MG_CARRY_MAX_JOBS);
    if (lanes < 1 || lanes > MG_REPAIR_MAX_LANES)
        return fail(ctx, MG_E_ARG, "carry_batch: %u lanes outside 1..%u", lanes,
                    MG_REPAIR_MAX_LANES);
    if (max_leaves > MG_CARRY_MAX_LEAVES)
        return fail(ctx, MG_E_ARG, "carry_batch: max_leaves %u above %u", max_leaves,
                    MG_CARRY_MAX_LEAVES);
    std::vector<uint32_t> n_leaves(n_jobs);
    uint32_t most = 0, max_lds = 0;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_carry_job& j = jobs[g];
        if (!j.prog) return fail(ctx, MG_E_ARG, "carry_batch: job %u: null program", g);
        if (j.prog->ctx != ctx)
            return fail(ctx, MG_E_ARG, "carry_batch: job %u: a program of another context", g);
        if (j.prog->n_leaves > max_leaves)
            return fail(ctx, MG_E_ARG, "carry_batch: job %u: %u leaves above max_leaves %u", g,
                        j.prog->n_leaves, max_leaves);
        if (j.prog->n_leaves && (!j.pin_rows || !j.pin_mask))
            return fail(ctx, MG_E_ARG, "carry_batch: job %u: null pin rows or pin mask", g);
        if (j.prog->leafgen.size() != j.prog->n_leaves ||
            !mg_carry_gen_ok(j.prog->leafgen.data(), j.prog->n_leaves, j.prog->n_consts))
            return fail(ctx, MG_E_ARG, "carry_batch: job %u: the program's leaf generators are "
                        "not loaded", g);
        n_leaves[g] = j.prog->n_leaves;
        most = n_leaves[g] > most ? n_leaves[g] : most;
        max_lds = j.prog->n_lds > max_lds ? j.prog->n_lds : max_lds;
    }
    std::vector<uint64_t> off(MG_CY_SHARED + (size_t)n_jobs * MG_CY_JOB_REGIONS);
    uint64_t bytes = 0, leaf_w = 0;
    if (!mg_carry_plan(n_leaves.data(), n_jobs, lanes, max_leaves, off.data(), &bytes, &leaf_w))
        return fail(ctx, MG_E_ARG, "carry_batch: the batch's buffer exceeds 64 bits");
    if (bytes > MG_WALK_BATCH_DEFAULT_BYTES)
        return fail(ctx, MG_E_ARG, "carry_batch: %llu bytes needed for %u jobs at %u lanes, at "
                    "most %llu; pass fewer jobs or lanes", (unsigned long long)bytes, n_jobs,
                    lanes, (unsigned long long)MG_WALK_BATCH_DEFAULT_BYTES);
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    void* ws;
    int rc = workspace(ctx, (size_t)bytes + 256, &ws);
    if (rc) return rc;
    uint8_t* w = (uint8_t*)ws;
    // the host image of everything uploaded, at the offsets of the plan
    const size_t up_b = (size_t)off[MG_CY_OUT];
    std::vector<uint8_t> img(up_b, 0);
    mg_pdesc* h_descs = (mg_pdesc*)(img.data() + off[MG_CY_DESCS]);
    mg_carry_dev_job* h_jobs = (mg_carry_dev_job*)(img.data() + off[MG_CY_JOBS]);
    memset(img.data() + off[MG_CY_FIRST], 0xFF, (size_t)n_jobs * 8);
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_carry_job& j = jobs[g];
        const uint32_t n = n_leaves[g];
        auto at = [&](uint32_t k) { return off[MG_CY_OFF(g, k)]; };
        if (n) {
            memcpy(img.data() + at(MG_CY_MASK), j.pin_mask, (size_t)((n + 31) / 32) * 4);
            memcpy(img.data() + at(MG_CY_ROWS), j.pin_rows, (size_t)n * 32);
            memcpy(img.data() + at(MG_CY_GEN), j.prog->leafgen.data(), (size_t)n * sizeof(mg_leafgen));
        }
        h_descs[g] = j.prog->h_desc;
        mg_carry_dev_job& d = h_jobs[g];
        d.mask = (const uint32_t*)(w + at(MG_CY_MASK));
        d.rows = (const uint32_t*)(w + at(MG_CY_ROWS));
        d.gen = (const mg_leafgen*)(w + at(MG_CY_GEN));
        d.consts = j.prog->h_desc.consts;              // the first n_consts entries: as loaded
        d.leaves = (uint32_t*)(w + at(MG_CY_LEAVES));
        d.prog_seed = j.prog->h_desc.prog_seed;
        d.n_leaves = n;
        d.n_rungs = 0;
    }
    const mg_pdesc* d_descs = (const mg_pdesc*)(w + off[MG_CY_DESCS]);
    const mg_carry_dev_job* d_jobs = (const mg_carry_dev_job*)(w + off[MG_CY_JOBS]);
    unsigned long long* d_first = (unsigned long long*)(w + off[MG_CY_FIRST]);
    long long* d_out_first = (long long*)(w + off[MG_CY_OUT]);
    uint32_t* d_out_leaves = (uint32_t*)(w + off[MG_CY_OUT] + (size_t)n_jobs * 8);
    HIPCHECK(ctx, hipMemcpyAsync(w, img.data(), up_b, hipMemcpyHostToDevice, ctx->stream));
    mg_run run = empty_run();
    run.leaves = (const uint32_t*)(w + off[MG_CY_OFF(0, MG_CY_LEAVES)]);
    run.leaves_prog_words = leaf_w;
    run.first_sat = d_first;                           // first_index 0: the lane itself
    run.stride = lanes;
    run.n_assign = lanes;
    timing_begin(ctx);
    HIPCHECK(ctx, mg_launch_carry_fill(d_jobs, n_jobs, most, gen->seed, gen->first_index, lanes,
                                       ctx->stream));
    HIPCHECK(ctx, launch(ctx, 0, d_descs, n_jobs, run, max_lds, ctx->stream));
    HIPCHECK(ctx, mg_launch_carry_gather(d_jobs, n_jobs, d_first, lanes, max_leaves, d_out_first,
                                         d_out_leaves, ctx->stream));
    timing_end(ctx);
    const size_t out_b = (size_t)n_jobs * 8 + (size_t)n_jobs * max_leaves * 32;
    std::vector<uint8_t> h_out(out_b);
    HIPCHECK(ctx, hipMemcpyAsync(h_out.data(), d_out_first, out_b, hipMemcpyDeviceToHost,
                                 ctx->stream));
    if (fill_out && leaf_w)
        HIPCHECK(ctx, hipMemcpyAsync(fill_out, run.leaves, (size_t)n_jobs * leaf_w * 4,
                                     hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    timing_read(ctx);
    memcpy(first, h_out.data(), (size_t)n_jobs * 8);
    memcpy(leaves, h_out.data() + (size_t)n_jobs * 8, (size_t)n_jobs * max_leaves * 32);
    return MG_OK;
}

int mg_carry_fill_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                       uint32_t n_consts, uint64_t prog_seed, const uint32_t* pin_rows,
                       const uint32_t* pin_mask, uint64_t seed, uint64_t first_index,
                       uint32_t lanes, uint32_t lane0, uint32_t n_lanes, uint32_t* out,
                       uint32_t* classes) {
    if (n_leaves == 0 || n_lanes == 0) return MG_OK;
    if (!leaves || !pin_rows || !pin_mask || !out || (n_consts && !consts)) return MG_E_ARG;
    if (lanes < 1 || lanes > MG_REPAIR_MAX_LANES || lane0 >= lanes || n_lanes > lanes - lane0)
        return MG_E_ARG;
    if (!mg_carry_gen_ok(leaves, n_leaves, n_consts)) return MG_E_ARG;
    for (uint32_t l = 0; l < n_leaves; ++l)
        for (uint32_t i = 0; i < n_lanes; ++i) {
            mg_carry_fill_lane(pin_mask, pin_rows, leaves, consts, prog_seed, seed, first_index, l,
                               lane0 + i, n_lanes, i, out);
            if (classes)
                classes[(size_t)l * n_lanes + i] = mg_carry_pinned(pin_mask, l) ? 0xFFFFFFFFu :
                    mg_carry_branch(leaves[l], mg_carry_class(seed, prog_seed, l,
                                                              first_index + lane0 + i));
        }
    return MG_OK;
}

int mg_carry_plan_host(const uint32_t* n_leaves, uint32_t n_jobs, uint32_t lanes,
                       uint32_t max_leaves, uint64_t* out_offsets, uint64_t* out_bytes,
                       uint64_t* out_leaf_stride_w) {
    return mg_carry_plan(n_leaves, n_jobs, lanes, max_leaves, out_offsets, out_bytes,
                         out_leaf_stride_w) ? MG_OK : MG_E_ARG;
}

// What mg_carry_ladder refuses of the shared counts and of one job
// (mg_carry_census asks the same); `who` begins the message.
static int carry_ladder_check_shared(mg_ctx* ctx, const char* who, uint32_t n_jobs,
                                     uint32_t lanes, uint32_t max_leaves) {
    if (n_jobs < 1 || n_jobs > MG_CARRY_MAX_JOBS)
        return fail(ctx, MG_E_ARG, "%s: %u jobs outside 1..%u", who, n_jobs, MG_CARRY_MAX_JOBS);
    if (lanes < 1 || lanes > MG_REPAIR_MAX_LANES)
        return fail(ctx, MG_E_ARG, "%s: %u lanes outside 1..%u", who, lanes, MG_REPAIR_MAX_LANES);
    if (max_leaves > MG_CARRY_MAX_LEAVES)
        return fail(ctx, MG_E_ARG, "%s: max_leaves %u above %u", who, max_leaves,
                    MG_CARRY_MAX_LEAVES);
    return MG_OK;
}

static int carry_ladder_check_job(mg_ctx* ctx, const char* who, uint32_t g,
                                  const mg_carry_ladder_job& j, uint32_t max_leaves) {
    if (!j.prog) return fail(ctx, MG_E_ARG, "%s: job %u: null program", who, g);
    if (j.prog->ctx != ctx)
        return fail(ctx, MG_E_ARG, "%s: job %u: a program of another context", who, g);
    if (j.prog->n_leaves > max_leaves)
        return fail(ctx, MG_E_ARG, "%s: job %u: %u leaves above max_leaves %u", who, g,
                    j.prog->n_leaves, max_leaves);
    if (j.n_rungs < 1 || j.n_rungs > MG_CARRY_MAX_RUNGS)
        return fail(ctx, MG_E_ARG, "%s: job %u: %u rungs outside 1..%u", who, g, j.n_rungs,
                    MG_CARRY_MAX_RUNGS);
    if (j.prog->n_leaves && (!j.pin_rows || !j.pin_masks))
        return fail(ctx, MG_E_ARG, "%s: job %u: null pin rows or pin masks", who, g);
    if (j.prog->leafgen.size() != j.prog->n_leaves ||
        !mg_carry_gen_ok(j.prog->leafgen.data(), j.prog->n_leaves, j.prog->n_consts))
        return fail(ctx, MG_E_ARG, "%s: job %u: the program's leaf generators are not loaded",
                    who, g);
    return MG_OK;
}

// The pin ladder (include/mythgpu.h mg_carry_ladder, DESIGN.md §3.19;
// csrc/mg_carry.h, mg_carry_ladder.hip): mg_carry_batch's sequence with
// n_rungs masks per job and the largest n_rungs x lanes columns.
int mg_carry_ladder(mg_ctx* ctx, const mg_carry_ladder_job* jobs, uint32_t n_jobs,
                    const mg_gen* gen, uint32_t lanes, int64_t* first, int64_t* rung,
                    uint32_t* leaves, uint32_t max_leaves, uint32_t* fill_out) {
    if (!ctx) return MG_E_ARG;
    if (!jobs || !gen || !first || !rung || !leaves)
        return fail(ctx, MG_E_ARG, "carry_ladder: null argument");
    int rc = carry_ladder_check_shared(ctx, "carry_ladder", n_jobs, lanes, max_leaves);
    if (rc != MG_OK) return rc;
    std::vector<uint32_t> n_leaves(n_jobs), n_rungs(n_jobs);
    uint32_t most = 0, max_lds = 0, top = 0;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_carry_ladder_job& j = jobs[g];
        rc = carry_ladder_check_job(ctx, "carry_ladder", g, j, max_leaves);
        if (rc != MG_OK) return rc;
        n_leaves[g] = j.prog->n_leaves;
        n_rungs[g] = j.n_rungs;
        most = n_leaves[g] > most ? n_leaves[g] : most;
        top = j.n_rungs > top ? j.n_rungs : top;
        max_lds = j.prog->n_lds > max_lds ? j.prog->n_lds : max_lds;
    }
    uint32_t cols = 0;
    if (!mg_carry_ladder_ok(n_rungs.data(), n_jobs, lanes, &cols))
        return fail(ctx, MG_E_ARG, "carry_ladder: %u rungs of %u lanes above %u columns", top,
                    lanes, MG_REPAIR_MAX_LANES);
    std::vector<uint64_t> off(MG_CY_SHARED + (size_t)n_jobs * MG_CY_JOB_REGIONS);
    uint64_t bytes = 0, leaf_w = 0;
    if (!mg_carry_ladder_plan(n_leaves.data(), n_rungs.data(), n_jobs, lanes, max_leaves,
                              off.data(), &bytes, &leaf_w))
        return fail(ctx, MG_E_ARG, "carry_ladder: the batch's buffer exceeds 64 bits");
    if (bytes > MG_WALK_BATCH_DEFAULT_BYTES)
        return fail(ctx, MG_E_ARG, "carry_ladder: %llu bytes needed for %u jobs at %u columns, "
                    "at most %llu; pass fewer jobs, rungs or lanes", (unsigned long long)bytes,
                    n_jobs, cols, (unsigned long long)MG_WALK_BATCH_DEFAULT_BYTES);
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    void* ws;
    rc = workspace(ctx, (size_t)bytes + 256, &ws);
    if (rc) return rc;
    uint8_t* w = (uint8_t*)ws;
    // the host image of everything uploaded, at the offsets of the plan
    const size_t up_b = (size_t)off[MG_CY_OUT];
    std::vector<uint8_t> img(up_b, 0);
    mg_pdesc* h_descs = (mg_pdesc*)(img.data() + off[MG_CY_DESCS]);
    mg_carry_dev_job* h_jobs = (mg_carry_dev_job*)(img.data() + off[MG_CY_JOBS]);
    memset(img.data() + off[MG_CY_FIRST], 0xFF, (size_t)n_jobs * 8);
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_carry_ladder_job& j = jobs[g];
        const uint32_t n = n_leaves[g];
        auto at = [&](uint32_t k) { return off[MG_CY_OFF(g, k)]; };
        if (n) {
            memcpy(img.data() + at(MG_CY_MASK), j.pin_masks,
                   (size_t)((n + 31) / 32) * 4 * j.n_rungs);
            memcpy(img.data() + at(MG_CY_ROWS), j.pin_rows, (size_t)n * 32);
            memcpy(img.data() + at(MG_CY_GEN), j.prog->leafgen.data(), (size_t)n * sizeof(mg_leafgen));
        }
        h_descs[g] = j.prog->h_desc;
        mg_carry_dev_job& d = h_jobs[g];
        d.mask = (const uint32_t*)(w + at(MG_CY_MASK));
        d.rows = (const uint32_t*)(w + at(MG_CY_ROWS));
        d.gen = (const mg_leafgen*)(w + at(MG_CY_GEN));
        d.consts = j.prog->h_desc.consts;              // the first n_consts entries: as loaded
        d.leaves = (uint32_t*)(w + at(MG_CY_LEAVES));
        d.prog_seed = j.prog->h_desc.prog_seed;
        d.n_leaves = n;
        d.n_rungs = j.n_rungs;
    }
    const mg_pdesc* d_descs = (const mg_pdesc*)(w + off[MG_CY_DESCS]);
    const mg_carry_dev_job* d_jobs = (const mg_carry_dev_job*)(w + off[MG_CY_JOBS]);
    unsigned long long* d_first = (unsigned long long*)(w + off[MG_CY_FIRST]);
    long long* d_out_first = (long long*)(w + off[MG_CY_OUT]);
    long long* d_out_rung = d_out_first + n_jobs;
    uint32_t* d_out_leaves = (uint32_t*)(w + off[MG_CY_OUT] + (size_t)n_jobs * 16);
    HIPCHECK(ctx, hipMemcpyAsync(w, img.data(), up_b, hipMemcpyHostToDevice, ctx->stream));
    mg_run run = empty_run();
    run.leaves = (const uint32_t*)(w + off[MG_CY_OFF(0, MG_CY_LEAVES)]);
    run.leaves_prog_words = leaf_w;
    run.first_sat = d_first;                           // first_index 0: the column itself
    run.stride = cols;
    run.n_assign = cols;
    timing_begin(ctx);
    HIPCHECK(ctx, mg_launch_carry_fill_rungs(d_jobs, n_jobs, most, gen->seed, gen->first_index,
                                             lanes, cols, ctx->stream));
    HIPCHECK(ctx, launch(ctx, 0, d_descs, n_jobs, run, max_lds, ctx->stream));
    HIPCHECK(ctx, mg_launch_carry_gather_rungs(d_jobs, n_jobs, d_first, lanes, cols, max_leaves,
                                               d_out_first, d_out_rung, d_out_leaves,
                                               ctx->stream));
    timing_end(ctx);
    const size_t out_b = (size_t)n_jobs * 16 + (size_t)n_jobs * max_leaves * 32;
    std::vector<uint8_t> h_out(out_b);
    HIPCHECK(ctx, hipMemcpyAsync(h_out.data(), d_out_first, out_b, hipMemcpyDeviceToHost,
                                 ctx->stream));
    if (fill_out && leaf_w)
        HIPCHECK(ctx, hipMemcpyAsync(fill_out, run.leaves, (size_t)n_jobs * leaf_w * 4,
                                     hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    timing_read(ctx);
    memcpy(first, h_out.data(), (size_t)n_jobs * 8);
    memcpy(rung, h_out.data() + (size_t)n_jobs * 8, (size_t)n_jobs * 8);
    memcpy(leaves, h_out.data() + (size_t)n_jobs * 16, (size_t)n_jobs * max_leaves * 32);
    return MG_OK;
}

int mg_carry_fill_rungs_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                             uint32_t n_consts, uint64_t prog_seed, const uint32_t* pin_rows,
                             const uint32_t* pin_masks, uint32_t n_rungs, uint64_t seed,
                             uint64_t first_index, uint32_t lanes, uint32_t cols, uint32_t col0,
                             uint32_t n_cols, uint32_t* out) {
    if (n_rungs < 1 || n_rungs > MG_CARRY_MAX_RUNGS) return MG_E_ARG;
    if (lanes < 1 || cols < lanes || cols > MG_REPAIR_MAX_LANES || col0 > cols ||
        n_cols > cols - col0)
        return MG_E_ARG;
    if (n_leaves == 0 || n_cols == 0) return MG_OK;
    if (!leaves || !pin_rows || !pin_masks || !out || (n_consts && !consts)) return MG_E_ARG;
    if (!mg_carry_gen_ok(leaves, n_leaves, n_consts)) return MG_E_ARG;
    const uint32_t words = (n_leaves + 31) / 32;
    for (uint32_t l = 0; l < n_leaves; ++l)
        for (uint32_t i = 0; i < n_cols; ++i)
            mg_carry_fill_rung_lane(pin_masks, words, n_rungs, pin_rows, leaves, consts, prog_seed,
                                    seed, first_index, l, col0 + i, lanes, n_cols, i, out);
    return MG_OK;
}

int mg_carry_ladder_plan_host(const uint32_t* n_leaves, const uint32_t* n_rungs, uint32_t n_jobs,
                              uint32_t lanes, uint32_t max_leaves, uint64_t* out_offsets,
                              uint64_t* out_bytes, uint64_t* out_leaf_stride_w) {
    return mg_carry_ladder_plan(n_leaves, n_rungs, n_jobs, lanes, max_leaves, out_offsets,
                                out_bytes, out_leaf_stride_w) ? MG_OK : MG_E_ARG;
}

// Witness sets on the pin ladder (include/mythgpu.h mg_carry_ladder_sets,
// DESIGN.md §3.21; csrc/mg_carry.h, mg_carry_sets.hip): mg_carry_ladder's
// sequence with n_sets row sets per job and a row set per rung.
int mg_carry_ladder_sets(mg_ctx* ctx, const mg_carry_sets_job* jobs, uint32_t n_jobs,
                         const mg_gen* gen, uint32_t lanes, int64_t* first, int64_t* rung,
                         uint32_t* leaves, uint32_t max_leaves, uint32_t* fill_out) {
    if (!ctx) return MG_E_ARG;
    if (!jobs || !gen || !first || !rung || !leaves)
        return fail(ctx, MG_E_ARG, "carry_sets: null argument");
    int rc = carry_ladder_check_shared(ctx, "carry_sets", n_jobs, lanes, max_leaves);
    if (rc != MG_OK) return rc;
    std::vector<uint32_t> n_leaves(n_jobs), n_rungs(n_jobs), n_sets(n_jobs);
    uint32_t most = 0, max_lds = 0, top = 0;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_carry_sets_job& j = jobs[g];
        const mg_carry_ladder_job as_ladder = {j.prog, j.pin_rows, j.pin_masks, j.n_rungs, 0};
        rc = carry_ladder_check_job(ctx, "carry_sets", g, as_ladder, max_leaves);
        if (rc != MG_OK) return rc;
        if (j.n_sets < 1 || j.n_sets > MG_CARRY_MAX_SETS)
            return fail(ctx, MG_E_ARG, "carry_sets: job %u: %u sets outside 1..%u", g, j.n_sets,
                        MG_CARRY_MAX_SETS);
        if (!j.rung_set) return fail(ctx, MG_E_ARG, "carry_sets: job %u: null rung_set", g);
        if (!mg_carry_rung_set_ok(j.rung_set, j.n_rungs, j.n_sets))
            return fail(ctx, MG_E_ARG, "carry_sets: job %u: a rung_set entry not below its %u "
                        "sets", g, j.n_sets);
        n_leaves[g] = j.prog->n_leaves;
        n_rungs[g] = j.n_rungs;
        n_sets[g] = j.n_sets;
        most = n_leaves[g] > most ? n_leaves[g] : most;
        top = j.n_rungs > top ? j.n_rungs : top;
        max_lds = j.prog->n_lds > max_lds ? j.prog->n_lds : max_lds;
    }
    uint32_t cols = 0;
    if (!mg_carry_sets_ok(n_rungs.data(), n_sets.data(), n_jobs, lanes, &cols))
        return fail(ctx, MG_E_ARG, "carry_sets: %u rungs of %u lanes above %u columns", top,
                    lanes, MG_REPAIR_MAX_LANES);
    std::vector<uint64_t> off(MG_CS_TABLE(n_jobs));
    uint64_t bytes = 0, leaf_w = 0;
    if (!mg_carry_sets_plan(n_leaves.data(), n_rungs.data(), n_sets.data(), n_jobs, lanes,
                            max_leaves, off.data(), &bytes, &leaf_w))
        return fail(ctx, MG_E_ARG, "carry_sets: the batch's buffer exceeds 64 bits");
    if (bytes > MG_WALK_BATCH_DEFAULT_BYTES)
        return fail(ctx, MG_E_ARG, "carry_sets: %llu bytes needed for %u jobs at %u columns, "
                    "at most %llu; pass fewer jobs, rungs or lanes", (unsigned long long)bytes,
                    n_jobs, cols, (unsigned long long)MG_WALK_BATCH_DEFAULT_BYTES);
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    void* ws;
    rc = workspace(ctx, (size_t)bytes + 256, &ws);
    if (rc) return rc;
    uint8_t* w = (uint8_t*)ws;
    // the host image of everything uploaded, at the offsets of the plan
    const size_t up_b = (size_t)off[MG_CY_OUT];
    std::vector<uint8_t> img(up_b, 0);
    mg_pdesc* h_descs = (mg_pdesc*)(img.data() + off[MG_CY_DESCS]);
    mg_carry_dev_job* h_jobs = (mg_carry_dev_job*)(img.data() + off[MG_CY_JOBS]);
    mg_carry_sets_dev_job* h_sjobs =
        (mg_carry_sets_dev_job*)(img.data() + off[MG_CS_BASE(n_jobs) + MG_CS_RECORDS]);
    memset(img.data() + off[MG_CY_FIRST], 0xFF, (size_t)n_jobs * 8);
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_carry_sets_job& j = jobs[g];
        const uint32_t n = n_leaves[g];
        auto at = [&](uint32_t k) { return off[MG_CY_OFF(g, k)]; };
        const uint64_t at_set = off[MG_CS_OFF(n_jobs, g, MG_CS_RUNG_SET)];
        if (n) {
            memcpy(img.data() + at(MG_CY_MASK), j.pin_masks,
                   (size_t)((n + 31) / 32) * 4 * j.n_rungs);
            memcpy(img.data() + at(MG_CY_ROWS), j.pin_rows, (size_t)n * 32 * j.n_sets);
            memcpy(img.data() + at(MG_CY_GEN), j.prog->leafgen.data(), (size_t)n * sizeof(mg_leafgen));
        }
        memcpy(img.data() + at_set, j.rung_set, (size_t)j.n_rungs * 4);
        h_descs[g] = j.prog->h_desc;
        mg_carry_dev_job& d = h_jobs[g];
        d.mask = (const uint32_t*)(w + at(MG_CY_MASK));
        d.rows = (const uint32_t*)(w + at(MG_CY_ROWS));
        d.gen = (const mg_leafgen*)(w + at(MG_CY_GEN));
        d.consts = j.prog->h_desc.consts;              // the first n_consts entries: as loaded
        d.leaves = (uint32_t*)(w + at(MG_CY_LEAVES));
        d.prog_seed = j.prog->h_desc.prog_seed;
        d.n_leaves = n;
        d.n_rungs = j.n_rungs;
        h_sjobs[g].rung_set = (const uint32_t*)(w + at_set);
        h_sjobs[g].n_sets = j.n_sets;
        h_sjobs[g].pad = 0;
    }
    const mg_pdesc* d_descs = (const mg_pdesc*)(w + off[MG_CY_DESCS]);
    const mg_carry_dev_job* d_jobs = (const mg_carry_dev_job*)(w + off[MG_CY_JOBS]);
    const mg_carry_sets_dev_job* d_sjobs =
        (const mg_carry_sets_dev_job*)(w + off[MG_CS_BASE(n_jobs) + MG_CS_RECORDS]);
    unsigned long long* d_first = (unsigned long long*)(w + off[MG_CY_FIRST]);
    long long* d_out_first = (long long*)(w + off[MG_CY_OUT]);
    long long* d_out_rung = d_out_first + n_jobs;
    uint32_t* d_out_leaves = (uint32_t*)(w + off[MG_CY_OUT] + (size_t)n_jobs * 16);
    HIPCHECK(ctx, hipMemcpyAsync(w, img.data(), up_b, hipMemcpyHostToDevice, ctx->stream));
    mg_run run = empty_run();
    run.leaves = (const uint32_t*)(w + off[MG_CY_OFF(0, MG_CY_LEAVES)]);
    run.leaves_prog_words = leaf_w;
    run.first_sat = d_first;                           // first_index 0: the column itself
    run.stride = cols;
    run.n_assign = cols;
    timing_begin(ctx);
    HIPCHECK(ctx, mg_launch_carry_fill_sets(d_jobs, d_sjobs, n_jobs, most, gen->seed,
                                            gen->first_index, lanes, cols, ctx->stream));
    HIPCHECK(ctx, launch(ctx, 0, d_descs, n_jobs, run, max_lds, ctx->stream));
    HIPCHECK(ctx, mg_launch_carry_gather_rungs(d_jobs, n_jobs, d_first, lanes, cols, max_leaves,
                                               d_out_first, d_out_rung, d_out_leaves,
                                               ctx->stream));
    timing_end(ctx);
    const size_t out_b = (size_t)n_jobs * 16 + (size_t)n_jobs * max_leaves * 32;
    std::vector<uint8_t> h_out(out_b);
    HIPCHECK(ctx, hipMemcpyAsync(h_out.data(), d_out_first, out_b, hipMemcpyDeviceToHost,
                                 ctx->stream));
    if (fill_out && leaf_w)
        HIPCHECK(ctx, hipMemcpyAsync(fill_out, run.leaves, (size_t)n_jobs * leaf_w * 4,
                                     hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    timing_read(ctx);
    memcpy(first, h_out.data(), (size_t)n_jobs * 8);
    memcpy(rung, h_out.data() + (size_t)n_jobs * 8, (size_t)n_jobs * 8);
    memcpy(leaves, h_out.data() + (size_t)n_jobs * 16, (size_t)n_jobs * max_leaves * 32);
    return MG_OK;
}

int mg_carry_fill_sets_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                            uint32_t n_consts, uint64_t prog_seed, const uint32_t* pin_rows,
                            const uint32_t* pin_masks, const uint32_t* rung_set, uint32_t n_rungs,
                            uint32_t n_sets, uint64_t seed, uint64_t first_index, uint32_t lanes,
                            uint32_t cols, uint32_t col0, uint32_t n_cols, uint32_t* out) {
    if (n_rungs < 1 || n_rungs > MG_CARRY_MAX_RUNGS) return MG_E_ARG;
    if (n_sets < 1 || n_sets > MG_CARRY_MAX_SETS || !mg_carry_rung_set_ok(rung_set, n_rungs, n_sets))
        return MG_E_ARG;
    if (lanes < 1 || cols < lanes || cols > MG_REPAIR_MAX_LANES || col0 > cols ||
        n_cols > cols - col0)
        return MG_E_ARG;
    if (n_leaves == 0 || n_cols == 0) return MG_OK;
    if (!leaves || !pin_rows || !pin_masks || !out || (n_consts && !consts)) return MG_E_ARG;
    if (!mg_carry_gen_ok(leaves, n_leaves, n_consts)) return MG_E_ARG;
    const uint32_t words = (n_leaves + 31) / 32;
    for (uint32_t l = 0; l < n_leaves; ++l)
        for (uint32_t i = 0; i < n_cols; ++i)
            mg_carry_fill_set_lane(pin_masks, words, n_rungs, rung_set, pin_rows, n_leaves, leaves,
                                   consts, prog_seed, seed, first_index, l, col0 + i, lanes,
                                   n_cols, i, out);
    return MG_OK;
}

int mg_carry_sets_plan_host(const uint32_t* n_leaves, const uint32_t* n_rungs,
                            const uint32_t* n_sets, uint32_t n_jobs, uint32_t lanes,
                            uint32_t max_leaves, uint64_t* out_offsets, uint64_t* out_bytes,
                            uint64_t* out_leaf_stride_w) {
    return mg_carry_sets_plan(n_leaves, n_rungs, n_sets, n_jobs, lanes, max_leaves, out_offsets,
                              out_bytes, out_leaf_stride_w) ? MG_OK : MG_E_ARG;
}

// The census of a pin ladder (include/mythgpu.h mg_carry_census, DESIGN.md
// §3.20; csrc/mg_carry.h, mg_carry_census.hip): the ladder's fill, the
// interpreter's launch writing every job's mask probes, a census per (job,
// rung) and the start columns, between one upload and one download.
int mg_carry_census(mg_ctx* ctx, const mg_carry_census_job* jobs, uint32_t n_jobs,
                    const mg_gen* gen, uint32_t lanes, uint32_t walkers, uint32_t max_roots,
                    uint32_t max_leaves, uint64_t* counts, int64_t* start_col,
                    uint32_t* start_nfail, uint32_t* starts, uint32_t* fill_out) {
    if (!ctx) return MG_E_ARG;
    if (!jobs || !gen || !counts || !start_col || !start_nfail || !starts)
        return fail(ctx, MG_E_ARG, "carry_census: null argument");
    int rc = carry_ladder_check_shared(ctx, "carry_census", n_jobs, lanes, max_leaves);
    if (rc != MG_OK) return rc;
    if (walkers < 1 || walkers > MG_CARRY_MAX_WALKERS)
        return fail(ctx, MG_E_ARG, "carry_census: %u walkers outside 1..%u", walkers,
                    MG_CARRY_MAX_WALKERS);
    std::vector<uint32_t> n_leaves(n_jobs), n_rungs(n_jobs), n_roots(n_jobs), n_probes(n_jobs),
        probe0(n_jobs);
    uint32_t most = 0, max_lds = 0, top = 0;
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_carry_census_job& j = jobs[g];
        rc = carry_ladder_check_job(ctx, "carry_census", g, j.ladder, max_leaves);
        if (rc != MG_OK) return rc;
        if (!mg_census_roots_ok(j.n_roots))
            return fail(ctx, MG_E_ARG, "carry_census: job %u: n_roots %u outside 1..%u", g,
                        j.n_roots, MG_CENSUS_MAX_ROOTS);
        if (j.n_roots > max_roots)
            return fail(ctx, MG_E_ARG, "carry_census: job %u: n_roots %u above max_roots %u", g,
                        j.n_roots, max_roots);
        if (!mg_census_mask_ok(j.ladder.prog->n_probes, j.n_roots, j.mask_probe0))
            return fail(ctx, MG_E_ARG, "carry_census: job %u: mask probes %u..%u outside the "
                        "program's %u probes", g, j.mask_probe0,
                        j.mask_probe0 + (j.n_roots + 255) / 256 - 1, j.ladder.prog->n_probes);
        n_leaves[g] = j.ladder.prog->n_leaves;
        n_rungs[g] = j.ladder.n_rungs;
        n_roots[g] = j.n_roots;
        n_probes[g] = j.ladder.prog->n_probes;
        probe0[g] = j.mask_probe0;
        most = n_leaves[g] > most ? n_leaves[g] : most;
        top = n_rungs[g] > top ? n_rungs[g] : top;
        max_lds = j.ladder.prog->n_lds > max_lds ? j.ladder.prog->n_lds : max_lds;
    }
    uint32_t cols = 0;
    if (!mg_carry_ladder_ok(n_rungs.data(), n_jobs, lanes, &cols))
        return fail(ctx, MG_E_ARG, "carry_census: %u rungs of %u lanes above %u columns", top,
                    lanes, MG_REPAIR_MAX_LANES);
    std::vector<uint64_t> off(MG_CC_TABLE(n_jobs));
    uint64_t bytes = 0, leaf_w = 0, probe_w = 0;
    if (mg_carry_census_plan(n_leaves.data(), n_rungs.data(), n_roots.data(), n_probes.data(),
                             probe0.data(), n_jobs, lanes, walkers, max_leaves, off.data(),
                             &bytes, &leaf_w, &probe_w, nullptr) != MG_CC_OK)
        return fail(ctx, MG_E_ARG, "carry_census: the batch's buffer exceeds 64 bits");
    if (bytes > MG_WALK_BATCH_DEFAULT_BYTES)
        return fail(ctx, MG_E_ARG, "carry_census: %llu bytes needed for %u jobs at %u columns "
                    "and %u walkers, at most %llu; pass fewer jobs, rungs, lanes or walkers",
                    (unsigned long long)bytes, n_jobs, cols, walkers,
                    (unsigned long long)MG_WALK_BATCH_DEFAULT_BYTES);
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    void* ws;
    rc = workspace(ctx, (size_t)bytes + 256, &ws);
    if (rc) return rc;
    uint8_t* w = (uint8_t*)ws;
    // the host image of everything uploaded, at the offsets of the plan; the
    // counters come back into it with the output block behind them
    const size_t up_b = (size_t)off[MG_CY_OUT];
    const size_t count0 = (size_t)off[MG_CC_OFF(n_jobs, 0, MG_CC_COUNTS)];
    const size_t out_b = (size_t)n_jobs * (size_t)mg_carry_census_out_job(walkers, max_leaves);
    std::vector<uint8_t> img(up_b + out_b, 0);
    mg_pdesc* h_descs = (mg_pdesc*)(img.data() + off[MG_CY_DESCS]);
    mg_carry_dev_job* h_jobs = (mg_carry_dev_job*)(img.data() + off[MG_CY_JOBS]);
    mg_carry_census_dev_job* h_cjobs =
        (mg_carry_census_dev_job*)(img.data() + off[MG_CC_BASE(n_jobs) + MG_CC_RECORDS]);
    for (uint32_t g = 0; g < n_jobs; ++g) {
        const mg_carry_ladder_job& j = jobs[g].ladder;
        const uint32_t n = n_leaves[g], roots = n_roots[g];
        auto at = [&](uint32_t k) { return off[MG_CY_OFF(g, k)]; };
        if (n) {
            memcpy(img.data() + at(MG_CY_MASK), j.pin_masks,
                   (size_t)((n + 31) / 32) * 4 * j.n_rungs);
            memcpy(img.data() + at(MG_CY_ROWS), j.pin_rows, (size_t)n * 32);
            memcpy(img.data() + at(MG_CY_GEN), j.prog->leafgen.data(), (size_t)n * sizeof(mg_leafgen));
        }
        h_descs[g] = j.prog->h_desc;
        mg_carry_dev_job& d = h_jobs[g];
        d.mask = (const uint32_t*)(w + at(MG_CY_MASK));
        d.rows = (const uint32_t*)(w + at(MG_CY_ROWS));
        d.gen = (const mg_leafgen*)(w + at(MG_CY_GEN));
        d.consts = j.prog->h_desc.consts;
        d.leaves = (uint32_t*)(w + at(MG_CY_LEAVES));
        d.prog_seed = j.prog->h_desc.prog_seed;
        d.n_leaves = n;
        d.n_rungs = j.n_rungs;
        mg_carry_census_dev_job& c = h_cjobs[g];
        c.mrows = (const uint32_t*)(w + off[MG_CC_OFF(n_jobs, g, MG_CC_PROBES)]) +
                  (size_t)probe0[g] * 8 * cols;
        c.counts = (unsigned long long*)(w + off[MG_CC_OFF(n_jobs, g, MG_CC_COUNTS)]);
        c.n_roots = roots;
        unsigned long long* h =
            (unsigned long long*)(img.data() + off[MG_CC_OFF(n_jobs, g, MG_CC_COUNTS)]);
        for (uint32_t r = 0; r < j.n_rungs; ++r)
            for (uint32_t k = mg_census_sole_index(roots); k < mg_census_words(roots); ++k)
                h[(size_t)r * mg_census_words(roots) + k] = ~0ull;
    }
    const mg_pdesc* d_descs = (const mg_pdesc*)(w + off[MG_CY_DESCS]);
    const mg_carry_dev_job* d_jobs = (const mg_carry_dev_job*)(w + off[MG_CY_JOBS]);
    const mg_carry_census_dev_job* d_cjobs =
        (const mg_carry_census_dev_job*)(w + off[MG_CC_BASE(n_jobs) + MG_CC_RECORDS]);
    long long* d_out_col = (long long*)(w + off[MG_CY_OUT]);
    uint32_t* d_out_nfail = (uint32_t*)(w + off[MG_CY_OUT] + (size_t)n_jobs * walkers * 8);
    uint32_t* d_out_rows = (uint32_t*)(w + off[MG_CY_OUT] + (size_t)n_jobs * walkers * 12);
    HIPCHECK(ctx, hipMemcpyAsync(w, img.data(), up_b, hipMemcpyHostToDevice, ctx->stream));
    mg_run run = empty_run();
    run.leaves = (const uint32_t*)(w + off[MG_CY_OFF(0, MG_CY_LEAVES)]);
    run.leaves_prog_words = leaf_w;
    run.probes = (uint32_t*)(w + off[MG_CC_OFF(n_jobs, 0, MG_CC_PROBES)]);
    run.probe_prog_words = probe_w;
    run.probes_per_prog = 1;
    run.stride = cols;
    run.n_assign = cols;
    timing_begin(ctx);
    HIPCHECK(ctx, mg_launch_carry_fill_rungs(d_jobs, n_jobs, most, gen->seed, gen->first_index,
                                             lanes, cols, ctx->stream));
    HIPCHECK(ctx, launch(ctx, 0, d_descs, n_jobs, run, max_lds, ctx->stream));
    HIPCHECK(ctx, mg_launch_carry_census(d_jobs, d_cjobs, n_jobs, top, lanes, cols, ctx->stream));
    HIPCHECK(ctx, mg_launch_carry_starts(d_jobs, d_cjobs, n_jobs, walkers, cols, max_leaves,
                                         d_out_col, d_out_nfail, d_out_rows, ctx->stream));
    timing_end(ctx);
    // the counter regions end where the output block begins: one copy
    HIPCHECK(ctx, hipMemcpyAsync(img.data() + count0, w + count0, up_b - count0 + out_b,
                                 hipMemcpyDeviceToHost, ctx->stream));
    if (fill_out && leaf_w)
        HIPCHECK(ctx, hipMemcpyAsync(fill_out, run.leaves, (size_t)n_jobs * leaf_w * 4,
                                     hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    timing_read(ctx);
    const size_t block_w = 5 * (size_t)max_roots + 2;
    memset(counts, 0, (size_t)n_jobs * top * block_w * 8);
    for (uint32_t g = 0; g < n_jobs; ++g)
        for (uint32_t r = 0; r < n_rungs[g]; ++r)
            memcpy(counts + ((size_t)g * top + r) * block_w,
                   img.data() + off[MG_CC_OFF(n_jobs, g, MG_CC_COUNTS)] +
                       (size_t)r * mg_census_words(n_roots[g]) * 8,
                   (size_t)mg_census_words(n_roots[g]) * 8);
    const uint8_t* h_out = img.data() + up_b;
    memcpy(start_col, h_out, (size_t)n_jobs * walkers * 8);
    memcpy(start_nfail, h_out + (size_t)n_jobs * walkers * 8, (size_t)n_jobs * walkers * 4);
    memcpy(starts, h_out + (size_t)n_jobs * walkers * 12,
           (size_t)n_jobs * walkers * max_leaves * 32);
    return MG_OK;
}

int mg_carry_census_plan_host(const uint32_t* n_leaves, const uint32_t* n_rungs,
                              const uint32_t* n_roots, const uint32_t* n_probes,
                              const uint32_t* mask_probe0, uint32_t n_jobs, uint32_t lanes,
                              uint32_t walkers, uint32_t max_leaves, uint64_t* out_offsets,
                              uint64_t* out_bytes, uint64_t* out_leaf_stride_w,
                              uint64_t* out_probe_stride_w) {
    return mg_carry_census_plan(n_leaves, n_rungs, n_roots, n_probes, mask_probe0, n_jobs, lanes,
                                walkers, max_leaves, out_offsets, out_bytes, out_leaf_stride_w,
                                out_probe_stride_w, nullptr) == MG_CC_OK ? MG_OK : MG_E_ARG;
}

int mg_carry_starts_host(const uint64_t* counts, uint32_t n_roots, uint32_t n_rungs,
                         uint32_t walkers, int64_t* start_col, uint32_t* start_nfail) {
    if (!counts || !start_col || !start_nfail) return MG_E_ARG;
    if (!mg_census_roots_ok(n_roots) || n_rungs < 1 || n_rungs > MG_CARRY_MAX_RUNGS ||
        walkers < 1 || walkers > MG_CARRY_MAX_WALKERS)
        return MG_E_ARG;
    mg_carry_pick_starts((const unsigned long long*)counts, n_roots, n_rungs, walkers, start_col,
                         start_nfail);
    return MG_OK;
}

// Host only: lanes lane0 .. lane0 + n_lanes - 1 of round r of the lane
// function of mg_walk_aim.h, as the mutate kernel writes them.
int mg_walk_aim_mutate_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                            uint32_t n_consts, const uint32_t* base, const uint32_t* rvals,
                            uint32_t n_resid, const uint32_t* entries, uint32_t n_entries,
                            const uint32_t* pieces, uint32_t n_pieces, uint64_t seed, uint32_t r,
                            uint32_t lanes, uint32_t lane0, uint32_t n_lanes, uint32_t* out,
                            uint32_t* moves) {
    if (!leaves || !base || !out || (n_consts && !consts) || n_leaves == 0) return MG_E_ARG;
    if (lanes < 1 || lanes > MG_REPAIR_MAX_LANES || r >= MG_REPAIR_MAX_ROUNDS) return MG_E_ARG;
    if (lane0 > lanes || n_lanes > lanes - lane0) return MG_E_ARG;
    for (uint32_t i = 0; i < n_leaves; ++i) {
        if (leaves[i].width < 1 || leaves[i].width > MG_MAX_WIDTH) return MG_E_ARG;
        if ((uint64_t)leaves[i].pool_off + leaves[i].pool_n > n_consts) return MG_E_ARG;
        uint32_t v[8];
        memcpy(v, base + (size_t)i * 8, 32);
        mg_repair_mask(v, leaves[i].width);
        if (memcmp(v, base + (size_t)i * 8, 32)) return MG_E_ARG;     // a base beyond its width
    }
    if (!mg_walk_aim_ok(entries, n_entries, pieces, n_pieces, leaves, n_leaves, n_resid))
        return MG_E_ARG;
    uint32_t live[MG_AIM_LIVE_WORDS];
    mg_walk_aim_live(entries, n_entries, rvals, live);
    for (uint32_t a = 0; a < n_lanes; ++a) {
        for (size_t i = 0; i < (size_t)n_leaves * 8; ++i) out[i * n_lanes + a] = base[i];
        mg_repair_moves mv;
        const uint32_t e = mg_walk_aim_lane(base, leaves, consts, n_leaves, seed, r, lane0 + a,
                                            lanes, entries, pieces, rvals, live, out + a, n_lanes,
                                            &mv);
        if (moves) {
            moves[5 * (size_t)a] = mv.n;
            moves[5 * (size_t)a + 1] = mv.kind[0] | mv.kind[1] << 8;
            moves[5 * (size_t)a + 2] = mv.leaf[0];
            moves[5 * (size_t)a + 3] = mv.leaf[1];
            moves[5 * (size_t)a + 4] = e;
        }
    }
    return MG_OK;
}

// Host only: what the three entries below share.  The argument and base
// checks, the validator of the rung (`rung`: 0 bound, 1 uf, 2 sum), then lanes
// lane0 .. lane0 + n_lanes - 1 of round r of the lane function of
// mg_walk_sum.h, as the mutate kernel writes them.  A lower rung passes empty
// UF tables, no destinations and mg_walk_no_lin.
static int walk_sum_mutate_host(int rung, const mg_leafgen* leaves, uint32_t n_leaves,
                                const uint32_t* consts, uint32_t n_consts, const uint32_t* base,
                                const uint32_t* rvals, uint32_t n_resid, const uint32_t* mvals,
                                uint32_t n_roots, uint32_t n_atoms, const uint32_t* entries,
                                uint32_t n_entries, const uint32_t* pieces, uint32_t n_pieces,
                                const uint32_t* fixed, const uint32_t* lin, const uint32_t* svals,
                                uint32_t n_srows, const mg_uf_tables& t, const uint32_t* dest,
                                uint64_t seed, uint32_t r, uint32_t lanes, uint32_t lane0,
                                uint32_t n_lanes, uint32_t* out, uint32_t* moves) {
    if (!leaves || !base || !out || (n_consts && !consts) || n_leaves == 0) return MG_E_ARG;
    if (lanes < 1 || lanes > MG_REPAIR_MAX_LANES || r >= MG_REPAIR_MAX_ROUNDS) return MG_E_ARG;
    if (lane0 > lanes || n_lanes > lanes - lane0) return MG_E_ARG;
    if (n_roots > MG_WT_MAX_ROOTS || n_atoms > MG_WT_MAX_ATOMS) return MG_E_ARG;
    if (t.n_slots && !dest) return MG_E_ARG;
    if (n_srows && rvals && mvals && !svals) return MG_E_ARG;
    for (uint32_t i = 0; i < n_leaves; ++i) {
        if (leaves[i].width < 1 || leaves[i].width > MG_MAX_WIDTH) return MG_E_ARG;
        if ((uint64_t)leaves[i].pool_off + leaves[i].pool_n > n_consts) return MG_E_ARG;
        uint32_t v[8];
        memcpy(v, base + (size_t)i * 8, 32);
        mg_repair_mask(v, leaves[i].width);
        if (memcmp(v, base + (size_t)i * 8, 32)) return MG_E_ARG;     // a base beyond its width
    }
    const bool ok =
        rung == 2 ? mg_walk_sum_ok(entries, n_entries, pieces, n_pieces, fixed, lin, n_srows, leaves,
                                   n_leaves, n_resid, n_roots, n_atoms, t)
        : rung == 1 ? mg_walk_uf_ok(entries, n_entries, pieces, n_pieces, fixed, leaves, n_leaves,
                                    n_resid, n_roots, n_atoms, t)
                    : mg_walk_bound_ok(entries, n_entries, pieces, n_pieces, fixed, leaves,
                                       n_leaves, n_resid, n_roots, n_atoms);
    if (!ok) return MG_E_ARG;
    for (uint32_t u = 0; u < t.n_slots; ++u)             // a destination is a leaf or none
        if (dest[u] != MG_AIM_NONE && dest[u] >= n_leaves) return MG_E_ARG;
    uint32_t live[MG_AIM_LIVE_WORDS];
    mg_walk_uf_live(entries, n_entries, pieces, rvals, mvals, MG_BOUND_MASK_WORDS(n_roots), dest,
                    live);
    for (uint32_t a = 0; a < n_lanes; ++a) {
        for (size_t i = 0; i < (size_t)n_leaves * 8; ++i) out[i * n_lanes + a] = base[i];
        mg_repair_moves mv;
        const uint32_t e = mg_walk_sum_lane(base, leaves, consts, n_leaves, seed, r, lane0 + a,
                                            lanes, entries, pieces, fixed, lin, rvals, svals,
                                            live, dest, out + a, n_lanes, &mv);
        if (moves) {
            moves[5 * (size_t)a] = mv.n;
            moves[5 * (size_t)a + 1] = mv.kind[0] | mv.kind[1] << 8;
            moves[5 * (size_t)a + 2] = mv.leaf[0];
            moves[5 * (size_t)a + 3] = mv.leaf[1];
            moves[5 * (size_t)a + 4] = e;
        }
    }
    return MG_OK;
}

// Host only: mg_walk_aim_mutate_host of the lane function of mg_walk_bound.h.
int mg_walk_bound_mutate_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                              uint32_t n_consts, const uint32_t* base, const uint32_t* rvals,
                              uint32_t n_resid, const uint32_t* mvals, uint32_t n_roots,
                              uint32_t n_atoms, const uint32_t* entries, uint32_t n_entries,
                              const uint32_t* pieces, uint32_t n_pieces, const uint32_t* fixed,
                              uint64_t seed, uint32_t r, uint32_t lanes, uint32_t lane0,
                              uint32_t n_lanes, uint32_t* out, uint32_t* moves) {
    return walk_sum_mutate_host(0, leaves, n_leaves, consts, n_consts, base, rvals, n_resid, mvals,
                                n_roots, n_atoms, entries, n_entries, pieces, n_pieces, fixed,
                                mg_walk_no_lin, nullptr, 0, mg_uf_tables{}, nullptr, seed, r,
                                lanes, lane0, n_lanes, out, moves);
}

// Host only: the destinations of the slots (mg_walk_uf_resolve of
// mg_walk_uf.h) under base ([n_leaves][8]) and U rows urows ([n_urows][8]),
// as the adopt kernel computes them; gen: the leaf table the validator reads.
int mg_walk_uf_resolve_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* base,
                            const uint32_t* urows, uint32_t n_urows, const uint32_t* slots,
                            uint32_t n_slots, const uint32_t* funcs, uint32_t n_funcs,
                            const uint32_t* cands, uint32_t n_cands, const uint32_t* ukeys,
                            uint32_t n_ukeys, uint32_t* dest) {
    if (!leaves || !base || n_leaves == 0 || (n_urows && !urows) || (n_slots && !dest))
        return MG_E_ARG;
    const mg_uf_tables t = {slots, n_slots, funcs, n_funcs, cands, n_cands, ukeys, n_ukeys,
                            n_urows};
    if (!mg_walk_uf_ok(nullptr, 0, nullptr, 0, nullptr, leaves, n_leaves, 0, 0, 0, t))
        return MG_E_ARG;
    for (uint32_t u = 0; u < n_slots; ++u)
        dest[u] = mg_walk_uf_resolve(slots, funcs, cands, ukeys, u, base, urows, 1);
    return MG_OK;
}

// Host only: mg_walk_bound_mutate_host of the lane function of mg_walk_uf.h;
// dest: the destinations of the n_slots slots under the base (any value when
// rvals or mvals is null: round 0).
int mg_walk_uf_mutate_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                           uint32_t n_consts, const uint32_t* base, const uint32_t* rvals,
                           uint32_t n_resid, const uint32_t* mvals, uint32_t n_roots,
                           uint32_t n_atoms, const uint32_t* entries, uint32_t n_entries,
                           const uint32_t* pieces, uint32_t n_pieces, const uint32_t* fixed,
                           const uint32_t* slots, uint32_t n_slots, const uint32_t* funcs,
                           uint32_t n_funcs, const uint32_t* cands, uint32_t n_cands,
                           const uint32_t* ukeys, uint32_t n_ukeys, uint32_t n_urows,
                           const uint32_t* dest, uint64_t seed, uint32_t r, uint32_t lanes,
                           uint32_t lane0, uint32_t n_lanes, uint32_t* out, uint32_t* moves) {
    const mg_uf_tables t = {slots, n_slots, funcs, n_funcs, cands, n_cands, ukeys, n_ukeys,
                            n_urows};
    return walk_sum_mutate_host(1, leaves, n_leaves, consts, n_consts, base, rvals, n_resid, mvals,
                                n_roots, n_atoms, entries, n_entries, pieces, n_pieces, fixed,
                                mg_walk_no_lin, nullptr, 0, t, dest, seed, r, lanes, lane0, n_lanes,
                                out, moves);
}

// Host only: mg_walk_uf_mutate_host of the lane function of mg_walk_sum.h;
// lin: the entries' lin words, svals: the side rows of the base ([n_srows][8];
// may be null when rvals or mvals is: round 0).
int mg_walk_sum_mutate_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                            uint32_t n_consts, const uint32_t* base, const uint32_t* rvals,
                            uint32_t n_resid, const uint32_t* mvals, uint32_t n_roots,
                            uint32_t n_atoms, const uint32_t* entries, uint32_t n_entries,
                            const uint32_t* pieces, uint32_t n_pieces, const uint32_t* fixed,
                            const uint32_t* lin, const uint32_t* svals, uint32_t n_srows,
                            const uint32_t* slots, uint32_t n_slots, const uint32_t* funcs,
                            uint32_t n_funcs, const uint32_t* cands, uint32_t n_cands,
                            const uint32_t* ukeys, uint32_t n_ukeys, uint32_t n_urows,
                            const uint32_t* dest, uint64_t seed, uint32_t r, uint32_t lanes,
                            uint32_t lane0, uint32_t n_lanes, uint32_t* out, uint32_t* moves) {
    const mg_uf_tables t = {slots, n_slots, funcs, n_funcs, cands, n_cands, ukeys, n_ukeys,
                            n_urows};
    return walk_sum_mutate_host(2, leaves, n_leaves, consts, n_consts, base, rvals, n_resid, mvals,
                                n_roots, n_atoms, entries, n_entries, pieces, n_pieces, fixed, lin,
                                svals, n_srows, t, dest, seed, r, lanes, lane0, n_lanes, out,
                                moves);
}

// Host only: the tree scoring (mg_walk_tree.h) on n lanes of host rows, as
// the score kernel runs it.  amasks may be null when there are no atoms.
int mg_walk_tree_score_host(const uint32_t* masks, const uint32_t* amasks, const uint32_t* resid,
                            const uint32_t* roots, uint32_t n_roots, const uint32_t* atoms,
                            uint32_t n_atoms, const uint32_t* code, uint32_t n_code,
                            uint32_t n_resid, uint64_t n, uint32_t* nfail, uint32_t* cost) {
    if (!masks || !roots || !nfail || !cost || (n_resid && !resid) || (n_atoms && !amasks))
        return MG_E_ARG;
    if (!mg_walk_tree_ok(roots, n_roots, atoms, n_atoms, code, n_code, n_resid)) return MG_E_ARG;
    uint32_t stack[MG_WT_STACK];
    for (uint64_t a = 0; a < n; ++a)
        mg_walk_tree_score_lane(masks, amasks, resid, n, a, roots, atoms, code, n_roots, true,
                                stack, 1, nfail + a, cost + a);
    return MG_OK;
}

// Host only: the scoring function (mg_walk.h) on n lanes of host rows, as
// the score kernel runs it.
int mg_walk_score_host(const uint32_t* masks, const uint32_t* resid, const uint32_t* table,
                       uint32_t n_roots, uint32_t n_resid, uint64_t n, uint32_t* nfail,
                       uint32_t* cost) {
    if (!masks || !table || !nfail || !cost || (n_resid && !resid)) return MG_E_ARG;
    if (n_roots < 1 || n_roots > MG_CENSUS_MAX_ROOTS || n_resid > 0xFFFFu) return MG_E_ARG;
    if (!walk_table_ok(table, n_roots, n_resid)) return MG_E_ARG;
    for (uint64_t a = 0; a < n; ++a)
        mg_walk_score_lane(masks, resid, n, a, table, n_roots, true, nfail + a, cost + a);
    return MG_OK;
}

int mg_batch_create(mg_ctx* ctx, const mg_prog* const* progs, uint32_t n_progs, mg_batch** out) {
    if (!ctx || !out || (n_progs && !progs)) return fail(ctx, MG_E_ARG, "null argument");
    *out = nullptr;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    std::vector<mg_pdesc> descs(n_progs);
    uint32_t max_lds = 0, max_leaves = 0, max_probes = 0;
    for (uint32_t i = 0; i < n_progs; ++i) {
        if (!progs[i] || progs[i]->ctx != ctx) return fail(ctx, MG_E_ARG, "program %u", i);
        descs[i] = progs[i]->h_desc;
        if (progs[i]->n_lds > max_lds) max_lds = progs[i]->n_lds;
        if (progs[i]->n_leaves > max_leaves) max_leaves = progs[i]->n_leaves;
        if (progs[i]->n_probes > max_probes) max_probes = progs[i]->n_probes;
    }
    mg_batch* b = new mg_batch();
    b->ctx = ctx;
    b->n = n_progs;
    b->max_lds = max_lds;
    b->max_leaves = max_leaves;
    b->max_probes = max_probes;
    if (n_progs) {
        void* d = nullptr;
        hipError_t e = dev_alloc(ctx, sizeof(mg_pdesc) * n_progs, &d, &b->descs_cls);
        b->d_descs = (mg_pdesc*)d;
        if (e == hipSuccess)
            e = hipMemcpy(b->d_descs, descs.data(), sizeof(mg_pdesc) * n_progs,
                          hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (b->d_descs) dev_release(ctx, b->d_descs, b->descs_cls);
            delete b;
            return fail(ctx, MG_E_HIP, "batch upload: %s", hipGetErrorString(e));
        }
    }
    *out = b;
    return MG_OK;
}

void mg_batch_free(mg_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    if (b->d_descs) dev_release(b->ctx, b->d_descs, b->descs_cls);
    delete b;
}

int mg_batch_eval_gen(mg_ctx* ctx, mg_batch* b, uint64_t seed, uint64_t first_index,
                      uint64_t n_assign, uint64_t* d_root_bits, uint64_t* d_first_sat,
                      void* stream) {
    if (!ctx || !b) return fail(ctx, MG_E_ARG, "null argument");
    if (b->ctx != ctx) return fail(ctx, MG_E_ARG, "batch belongs to another context");
    // like every other entry point: the caller's thread may have another
    // device current (two contexts on two devices driven from one thread)
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const uint64_t words = (n_assign + 63) / 64;
    for (uint32_t p0 = 0; p0 < b->n; p0 += 65535) {
        const uint32_t np = b->n - p0 < 65535 ? b->n - p0 : 65535;
        mg_run run = empty_run();
        run.n_assign = n_assign;
        run.stride = n_assign;
        run.words_per_prog = words;
        run.root_bits = d_root_bits ? d_root_bits + (size_t)p0 * words : nullptr;
        run.first_sat = d_first_sat ? (unsigned long long*)d_first_sat + p0 : nullptr;
        run.seed = seed;
        run.first_index = first_index;
        HIPCHECK(ctx, launch(ctx, 1, b->d_descs + p0, np, run, b->max_lds, s));
    }
    if (s != ctx->stream) HIPCHECK(ctx, ext_launched(ctx, s));
    return MG_OK;
}

int mg_batch_search(mg_ctx* ctx, mg_batch* b, const mg_gen* gen, uint64_t n_cand,
                    int64_t* first_sat, uint32_t* witness_leaves, uint32_t max_leaves) {
    return mg_batch_search_probes(ctx, b, gen, n_cand, first_sat, witness_leaves, max_leaves,
                                  nullptr, 0);
}

int mg_batch_search_probes(mg_ctx* ctx, mg_batch* b, const mg_gen* gen, uint64_t n_cand,
                           int64_t* first_sat, uint32_t* witness_leaves, uint32_t max_leaves,
                           uint32_t* witness_probes, uint32_t max_probes) {
    if (!ctx || !b || !gen || (b->n && !first_sat)) return fail(ctx, MG_E_ARG, "null argument");
    if (b->ctx != ctx) return fail(ctx, MG_E_ARG, "batch belongs to another context");
    if (witness_leaves && max_leaves < b->max_leaves)
        return fail(ctx, MG_E_ARG, "witness rows hold %u leaves, a program has %u", max_leaves,
                    b->max_leaves);
    if (witness_probes && (!witness_leaves || max_probes < b->max_probes))
        return fail(ctx, MG_E_ARG, "probe rows hold %u probes, a program has %u", max_probes,
                    b->max_probes);
    for (uint32_t i = 0; i < b->n; ++i) first_sat[i] = -1;
    if (n_cand == 0 || b->n == 0) return MG_OK;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    const size_t first_b = ((size_t)b->n * 8 + 255) & ~(size_t)255;
    const size_t wit_b = witness_leaves ? (size_t)b->n * max_leaves * 8 * 4 : 0;
    const size_t wit_b_al = (wit_b + 255) & ~(size_t)255;
    const size_t prb_b = witness_probes ? (size_t)b->n * max_probes * 8 * 4 : 0;
    void* ws;
    int rc = workspace(ctx, first_b + wit_b_al + prb_b, &ws);
    if (rc) return rc;
    unsigned long long* d_first = (unsigned long long*)ws;
    HIPCHECK(ctx, hipMemsetAsync(d_first, 0xFF, (size_t)b->n * 8, ctx->stream));
    timing_begin(ctx);
    // every program's whole candidate range, queued with no host round trip;
    // waves of solved programs exit at once (skip_solved)
    for (uint64_t done = 0; done < n_cand; done += MG_SEARCH_LAUNCH) {
        for (uint32_t p0 = 0; p0 < b->n; p0 += 65535) {
            const uint32_t np = b->n - p0 < 65535 ? b->n - p0 : 65535;
            mg_run run = empty_run();
            run.n_assign = n_cand - done < MG_SEARCH_LAUNCH ? n_cand - done : MG_SEARCH_LAUNCH;
            run.stride = run.n_assign;
            run.first_sat = d_first + p0;
            run.seed = gen->seed;
            run.first_index = gen->first_index + done;
            run.skip_solved = 1;
            HIPCHECK(ctx, launch(ctx, 1, b->d_descs + p0, np, run, b->max_lds, ctx->stream));
        }
    }
    timing_end(ctx);
    if (witness_leaves) {
        // one launch regenerates every program's winning candidate: lane 0
        // of program p evaluates candidate first_sat[p] (solved programs only)
        // (and, when asked, its probe values: what a solve-mode witness
        // computes besides the generated leaves)
        uint32_t* d_wit = (uint32_t*)((uint8_t*)ws + first_b);
        uint32_t* d_prb = prb_b ? (uint32_t*)((uint8_t*)ws + first_b + wit_b_al) : nullptr;
        HIPCHECK(ctx, hipMemsetAsync(d_wit, 0, wit_b, ctx->stream));
        if (prb_b) HIPCHECK(ctx, hipMemsetAsync(d_prb, 0, prb_b, ctx->stream));
        for (uint32_t p0 = 0; p0 < b->n; p0 += 65535) {
            const uint32_t np = b->n - p0 < 65535 ? b->n - p0 : 65535;
            mg_run run = empty_run();
            run.n_assign = 1;
            run.stride = 1;
            run.seed = gen->seed;
            run.first_per_prog = (const uint64_t*)(d_first + p0);
            run.leaves_out = d_wit + (size_t)p0 * max_leaves * 8;
            run.lout_prog_words = (uint64_t)max_leaves * 8;
            if (d_prb) {
                run.probes = d_prb + (size_t)p0 * max_probes * 8;
                run.probe_prog_words = (uint64_t)max_probes * 8;
            }
            HIPCHECK(ctx, launch(ctx, 1, b->d_descs + p0, np, run, b->max_lds, ctx->stream));
        }
        HIPCHECK(ctx, hipMemcpyAsync(witness_leaves, d_wit, wit_b, hipMemcpyDeviceToHost,
                                     ctx->stream));
        if (prb_b)
            HIPCHECK(ctx, hipMemcpyAsync(witness_probes, d_prb, prb_b, hipMemcpyDeviceToHost,
                                         ctx->stream));
    }
    std::vector<unsigned long long> h(b->n, ~0ull);
    HIPCHECK(ctx, hipMemcpyAsync(h.data(), d_first, (size_t)b->n * 8, hipMemcpyDeviceToHost,
                                 ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    timing_read(ctx);
    for (uint32_t i = 0; i < b->n; ++i) first_sat[i] = h[i] == ~0ull ? -1 : (int64_t)h[i];
    return MG_OK;
}

// The regeneration launch above with caller-given indices:
// lane 0 of pair i evaluates candidate indices[i] of progs[i].  The
// descriptor table is built per call, one copy per pair, in the workspace.
int mg_batch_witness(mg_ctx* ctx, const mg_prog* const* progs, const int64_t* indices, uint32_t n,
                     uint64_t seed, uint32_t* leaves, uint32_t max_leaves, uint32_t* probes,
                     uint32_t max_probes) {
    if (!ctx) return MG_E_ARG;
    if (n && (!progs || !indices || !leaves))
        return fail(ctx, MG_E_ARG, "batch_witness: null argument");
    uint32_t max_lds = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!progs[i]) return fail(ctx, MG_E_ARG, "batch_witness: pair %u: null program", i);
        if (progs[i]->ctx != ctx)
            return fail(ctx, MG_E_ARG, "batch_witness: pair %u: a program of another context", i);
        if (indices[i] < -1)
            return fail(ctx, MG_E_ARG, "batch_witness: pair %u: index %lld", i,
                        (long long)indices[i]);
        if (progs[i]->n_leaves > max_leaves)
            return fail(ctx, MG_E_ARG, "batch_witness: pair %u: leaf rows hold %u leaves, the "
                        "program has %u", i, max_leaves, progs[i]->n_leaves);
        if (probes && progs[i]->n_probes > max_probes)
            return fail(ctx, MG_E_ARG, "batch_witness: pair %u: probe rows hold %u probes, the "
                        "program has %u", i, max_probes, progs[i]->n_probes);
        if (progs[i]->n_lds > max_lds) max_lds = progs[i]->n_lds;
    }
    if (n == 0) return MG_OK;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    const size_t desc_b = ((size_t)n * sizeof(mg_pdesc) + 255) & ~(size_t)255;
    const size_t first_b = ((size_t)n * 8 + 255) & ~(size_t)255;
    const size_t wit_b = (size_t)n * max_leaves * 8 * 4;
    const size_t wit_b_al = (wit_b + 255) & ~(size_t)255;
    const size_t prb_b = probes ? (size_t)n * max_probes * 8 * 4 : 0;
    void* ws;
    int rc = workspace(ctx, desc_b + first_b + wit_b_al + prb_b + 256, &ws);
    if (rc) return rc;
    uint8_t* w = (uint8_t*)ws;
    // descriptors and indices in one upload (-1 is ~0: the pair's program returns)
    std::vector<uint8_t> img(desc_b + first_b, 0);
    mg_pdesc* h_descs = (mg_pdesc*)img.data();
    uint64_t* h_first = (uint64_t*)(img.data() + desc_b);
    for (uint32_t i = 0; i < n; ++i) {
        h_descs[i] = progs[i]->h_desc;
        h_first[i] = indices[i] < 0 ? ~0ull : (uint64_t)indices[i];
    }
    HIPCHECK(ctx, hipMemcpyAsync(w, img.data(), img.size(), hipMemcpyHostToDevice, ctx->stream));
    const mg_pdesc* d_descs = (const mg_pdesc*)w;
    const uint64_t* d_first = (const uint64_t*)(w + desc_b);
    uint32_t* d_wit = (uint32_t*)(w + desc_b + first_b);
    uint32_t* d_prb = prb_b ? (uint32_t*)(w + desc_b + first_b + wit_b_al) : nullptr;
    if (wit_b) HIPCHECK(ctx, hipMemsetAsync(d_wit, 0, wit_b, ctx->stream));
    if (prb_b) HIPCHECK(ctx, hipMemsetAsync(d_prb, 0, prb_b, ctx->stream));
    timing_begin(ctx);
    for (uint32_t p0 = 0; p0 < n; p0 += 65535) {
        const uint32_t np = n - p0 < 65535 ? n - p0 : 65535;
        mg_run run = empty_run();
        run.n_assign = 1;
        run.stride = 1;
        run.seed = seed;
        run.first_per_prog = d_first + p0;
        run.leaves_out = d_wit + (size_t)p0 * max_leaves * 8;
        run.lout_prog_words = (uint64_t)max_leaves * 8;
        if (d_prb) {
            run.probes = d_prb + (size_t)p0 * max_probes * 8;
            run.probe_prog_words = (uint64_t)max_probes * 8;
        }
        HIPCHECK(ctx, launch(ctx, 1, d_descs + p0, np, run, max_lds, ctx->stream));
    }
    timing_end(ctx);
    if (wit_b)
        HIPCHECK(ctx, hipMemcpyAsync(leaves, d_wit, wit_b, hipMemcpyDeviceToHost, ctx->stream));
    if (prb_b)
        HIPCHECK(ctx, hipMemcpyAsync(probes, d_prb, prb_b, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    timing_read(ctx);
    return MG_OK;
}

// The byte range of the executable sections of a code object and the
// address of its mg_jit_table symbol (both as link-time virtual addresses),
// read from the ELF itself with every offset bounds-checked: the entries an
// image names must lie in its code.
struct jit_layout {
    std::vector<std::pair<uint64_t, uint64_t>> text;   // [begin, end) of SHF_EXECINSTR sections
    uint64_t table = 0;
    bool found = false;
};

static bool elf_layout(const uint8_t* img, size_t n, jit_layout* out) {
    if (n < sizeof(Elf64_Ehdr) || memcmp(img, ELFMAG, SELFMAG) != 0 || img[EI_CLASS] != ELFCLASS64)
        return false;
    Elf64_Ehdr eh;
    memcpy(&eh, img, sizeof eh);
    if (eh.e_shentsize != sizeof(Elf64_Shdr) || eh.e_shoff > n ||
        (uint64_t)eh.e_shnum * sizeof(Elf64_Shdr) > n - eh.e_shoff)
        return false;
    std::vector<Elf64_Shdr> sh(eh.e_shnum);
    if (eh.e_shnum) memcpy(sh.data(), img + eh.e_shoff, eh.e_shnum * sizeof(Elf64_Shdr));
    for (const Elf64_Shdr& s : sh)
        if ((s.sh_flags & SHF_EXECINSTR) && s.sh_size)
            out->text.push_back({s.sh_addr, s.sh_addr + s.sh_size});
    for (const Elf64_Shdr& s : sh) {
        if ((s.sh_type != SHT_SYMTAB && s.sh_type != SHT_DYNSYM) || s.sh_link >= sh.size() ||
            s.sh_entsize != sizeof(Elf64_Sym) || s.sh_offset > n || s.sh_size > n - s.sh_offset)
            continue;
        const Elf64_Shdr& st = sh[s.sh_link];
        if (st.sh_offset > n || st.sh_size > n - st.sh_offset) continue;
        const char* names = (const char*)img + st.sh_offset;
        for (uint64_t k = 0; k < s.sh_size / sizeof(Elf64_Sym); ++k) {
            Elf64_Sym sym;
            memcpy(&sym, img + s.sh_offset + k * sizeof(Elf64_Sym), sizeof sym);
            static const char want[] = "mg_jit_table";
            if (sym.st_name + sizeof want > st.sh_size) continue;
            if (memcmp(names + sym.st_name, want, sizeof want) == 0) {
                out->table = sym.st_value;
                out->found = true;
                return true;
            }
        }
    }
    return true;
}

// Compiled programs: load the code object, read its entry table
// (mg_jit_table: a header row (MG_JIT_MAGIC, the asm digest of the
// interpreter the code was generated with: pinned registers, descriptor
// layout), then per program its entry relative to the table and its records'
// fingerprint) and point the programs' descriptors at their code.  Batches
// created afterwards copy the entries; the interpreter kernel then calls the
// code instead of dispatching records.  Every entry must lie inside an
// executable section of the image (read from its ELF headers) so a malformed
// image cannot send the kernel to an arbitrary address.
int mg_jit_attach(mg_ctx* ctx, mg_prog* const* progs, uint32_t n_progs, const void* image,
                  size_t image_size, mg_jit** out) {
    if (!ctx || !out || !image || !image_size || (n_progs && !progs))
        return fail(ctx, MG_E_ARG, "null argument");
    *out = nullptr;
    for (uint32_t i = 0; i < n_progs; ++i)
        if (!progs[i] || progs[i]->ctx != ctx) return fail(ctx, MG_E_ARG, "program %u", i);
    jit_layout lay;
    if (!elf_layout((const uint8_t*)image, image_size, &lay) || !lay.found || lay.text.empty())
        return fail(ctx, MG_E_ARG, "JIT image: not a code object with mg_jit_table and code");
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    hipModule_t mod = nullptr;
    HIPCHECK(ctx, hipModuleLoadData(&mod, image));
    hipDeviceptr_t d_table = nullptr;
    size_t table_b = 0;
    hipError_t e = hipModuleGetGlobal(&d_table, &table_b, mod, "mg_jit_table");
    // row 0: header; rows 1..n: (entry - table, records' fingerprint)
    std::vector<int64_t> row(2 * ((size_t)n_progs + 1));
    if (e == hipSuccess && table_b != ((size_t)n_progs + 1) * 16) e = hipErrorInvalidValue;
    if (e == hipSuccess) e = hipMemcpy(row.data(), d_table, table_b, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        (void)hipModuleUnload(mod);
        return fail(ctx, MG_E_HIP, "JIT image: %s (table %zu bytes for %u programs)",
                    hipGetErrorString(e), table_b, n_progs);
    }
    const uint64_t want_digest = strtoull(mg_asm_digest_layout(ctx->nreg), nullptr, 16);
    if ((uint64_t)row[0] != MG_JIT_MAGIC || (uint64_t)row[1] != want_digest) {
        (void)hipModuleUnload(mod);
        return fail(ctx, MG_E_ARG, "JIT image: built for another interpreter (header %016llx, "
                    "asm digest %016llx; this library %016llx)", (unsigned long long)row[0],
                    (unsigned long long)row[1], (unsigned long long)want_digest);
    }
    for (uint32_t i = 0; i < n_progs; ++i) {
        const int64_t rel = row[2 * (i + 1)];
        const uint64_t fp = (uint64_t)row[2 * (i + 1) + 1];
        if (rel == 0 && fp == 0) continue;                  // not compiled: interpreter
        const uint64_t at = lay.table + (uint64_t)rel;
        bool inside = false;
        for (const auto& t : lay.text) inside |= at >= t.first && at + 4 <= t.second;
        if (!inside || (rel & 3)) {
            (void)hipModuleUnload(mod);
            return fail(ctx, MG_E_ARG, "JIT image: entry %u at %lld outside the code", i,
                        (long long)rel);
        }
        if (fp != progs[i]->rec_fp) {
            (void)hipModuleUnload(mod);
            return fail(ctx, MG_E_ARG, "JIT image: entry %u was compiled for other records "
                        "(fingerprint %016llx, loaded program %016llx)", i,
                        (unsigned long long)fp, (unsigned long long)progs[i]->rec_fp);
        }
    }
    mg_jit* j = new mg_jit();
    j->ctx = ctx;
    j->module = mod;
    for (uint32_t i = 0; i < n_progs; ++i) {
        if (row[2 * (i + 1)] == 0) continue;                // stays on the interpreter
        const uint64_t entry = (uint64_t)(uintptr_t)d_table + (uint64_t)row[2 * (i + 1)];
        e = hipMemcpy((uint8_t*)progs[i]->d_desc + offsetof(mg_pdesc, jit_entry), &entry,
                      sizeof entry, hipMemcpyHostToDevice);
        if (e == hipSuccess) memcpy(&progs[i]->h_desc.jit_entry, &entry, sizeof entry);
        if (e != hipSuccess) {
            mg_jit_detach(j);
            return fail(ctx, MG_E_HIP, "JIT attach: %s", hipGetErrorString(e));
        }
        if (progs[i]->jit && progs[i]->jit != j) {    // re-attached: the old image lets go
            auto& v = progs[i]->jit->progs;
            v.erase(std::remove(v.begin(), v.end(), progs[i]), v.end());
        }
        progs[i]->jit = j;
        j->progs.push_back(progs[i]);
    }
    *out = j;
    return MG_OK;
}

// Back to the interpreter for every attached program (their descriptors'
// entries cleared), then the code object is unloaded.  Batches created while
// attached keep stale entries: free them first.
void mg_jit_detach(mg_jit* j) {
    if (!j) return;
    (void)hipSetDevice(j->ctx->device);
    const uint64_t zero = 0;
    for (mg_prog* p : j->progs) {
        (void)hipMemcpy((uint8_t*)p->d_desc + offsetof(mg_pdesc, jit_entry), &zero, sizeof zero,
                        hipMemcpyHostToDevice);
        memcpy(&p->h_desc.jit_entry, &zero, sizeof zero);
        p->jit = nullptr;
    }
    (void)hipDeviceSynchronize();
    if (j->module) (void)hipModuleUnload(j->module);
    delete j;
}

int mg_keccak256(mg_ctx* ctx, const uint8_t* data, const uint64_t* offsets, const uint32_t* lens,
                 uint32_t n, uint8_t* out) {
    if (!ctx || (n && (!offsets || !lens || !out))) return fail(ctx, MG_E_ARG, "null argument");
    if (n == 0) return MG_OK;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t end = offsets[i] + lens[i];
        if (end > total) total = end;
    }
    if (total && !data) return fail(ctx, MG_E_ARG, "null data");
    const size_t off_b = (size_t)n * 8, len_b = (size_t)n * 4, out_b = (size_t)n * 32;
    void* ws;
    int rc = workspace(ctx, total + off_b + len_b + out_b + 1024, &ws);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)ws;
    uint64_t* d_off = (uint64_t*)base;
    uint32_t* d_len = (uint32_t*)(base + off_b);
    uint8_t* d_out = base + ((off_b + len_b + 255) & ~(size_t)255);
    uint8_t* d_data = d_out + ((out_b + 255) & ~(size_t)255);
    HIPCHECK(ctx, hipMemcpyAsync(d_off, offsets, off_b, hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(ctx, hipMemcpyAsync(d_len, lens, len_b, hipMemcpyHostToDevice, ctx->stream));
    if (total)
        HIPCHECK(ctx, hipMemcpyAsync(d_data, data, total, hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(ctx, mg_launch_keccak(d_data, d_off, d_len, n, d_out, ctx->stream));
    HIPCHECK(ctx, hipMemcpyAsync(out, d_out, out_b, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MG_OK;
}

}  // extern "C"

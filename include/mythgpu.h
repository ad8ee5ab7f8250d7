/*
 * libmythgpu — C ABI of the MI355X batched constraint-evaluation engine.
 *
 * Drop-in boundary: the reference's only solver entry point is
 *   mythril/support/model.py:15-49   get_model(constraints, minimize, maximize,
 *                                              enforce_execution_time)
 * which builds a z3.Optimize and calls check()/model() through
 *   mythril/laser/smt/solver/solver.py:47-64  BaseSolver.check / .model.
 * The Python shim (mythril_amd/model.py) keeps get_model's signature and
 * contract and calls this library through ctypes for the witness search; the
 * entries below replace, respectively:
 *   mg_load_program   — Optimize.add(constraints)       solver.py:28-37
 *   mg_search         — Optimize.check() (SAT side)     solver.py:47-57
 *   mg_eval*          — Model.eval over many models     laser/smt/model.py:44-59
 *   mg_keccak256      — find_concrete_keccak            keccak_function_manager.py:43-57
 *
 * All pointers are caller-owned.  Functions return 0 on success and a
 * negative MG_E* code on failure (message: mg_last_error).  No exceptions
 * cross the ABI.  Calls on one mg_ctx are synchronous unless they take a
 * stream argument; use one mg_ctx per host thread.
 */
#ifndef MYTHGPU_H
#define MYTHGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_OK 0
#define MG_E_ARG (-1)      /* invalid argument / malformed program          */
#define MG_E_HIP (-2)      /* HIP runtime error                              */
#define MG_E_NODEV (-3)    /* no usable GPU                                  */
#define MG_E_NOMEM (-4)

typedef struct mg_ctx mg_ctx;
typedef struct mg_prog mg_prog;
typedef struct mg_batch mg_batch;
typedef struct mg_jit mg_jit;

/* Device candidate generator for one leaf (free variable / table cell),
 * generator v9 (restated bit-exactly by oracle/gen_ref.py):
 *   salt = prog_seed * 0xD1B54A32D192ED03 ^ (leaf + 1) * 0x8CB92BA72F3D8DD7
 *   ss   = seed ^ salt
 *   s    = (ss ^ index) + 0x9E3779B97F4A7C15        (mod 2^64)
 *   z    = (s ^ (s >> 32)) * 0xBF58476D1CE4E5B9     (mod 2^64)
 *   r0   = z ^ (z >> 32)                            (v5-v8: SplitMix64(ss ^ index))
 *   x    = lo(r0) ^ hi(r0)                          (32 bits)
 *   cls  = mulhi(((lo32(index >> 6) ^ lo32(ss)) * 0x2545F491 mod 2^32)
 *                ^ hi32(ss), 100)                   (one class per leaf per
 *                                                    group of 64 indices: a
 *                                                    wave from a multiple of
 *                                                    64 runs one class's code)
 * and by class (thresholds are cumulative percentages):
 *   pct_uniform <= cls < pct_small   r0 (< 2^64)
 *   pct_small <= cls < pct_boundary  {0, 1, 2^(w-1), 2^256-1, 2^k+1, 2^k-1},
 *                                    kind = mulhi(lo, 6), k = mulhi(lo * 0x9E3779B1, w)
 *   cls >= pct_boundary, pool_n > 0  consts[pool_off + e] + delta - 1,
 *                                    e = mulhi(lo, pool_n), delta = mulhi(lo * 0x85EBCA6B, 3)
 *   otherwise (uniform)              r0 in limbs 0-1; limb pair k = 1..3 is
 *                                    x * C_k + r0 (mod 2^64), C = 0x85EBCA6B,
 *                                    0xC2B2AE35, 0x27D4EB2F
 * every value masked to the leaf's width. */
typedef struct mg_leafgen {
    uint32_t width;
    uint32_t pool_off;
    uint32_t pool_n;
    uint32_t pct_uniform;
    uint32_t pct_small;
    uint32_t pct_boundary;
} mg_leafgen;

typedef struct mg_gen {
    uint64_t seed;          /* stream seed                                  */
    uint64_t first_index;   /* candidate index of the first lane (sharding) */
} mg_gen;

/* One context per (device, host thread).  SURVEY §8b proposed
 * mg_init(uint32_t device_mask, ...) with one context owning several devices;
 * this ABI deliberately takes ONE device index instead:
 *   - the multi-GPU design is one process per GPU (bench.py under
 *     torch.distributed.run) or, inside one process, one context per device
 *     driven from its own host thread (mythril_amd/model.py
 *     batch_search_devices: the C calls release the GIL), so a context never
 *     has to fan a call out over devices itself;
 *   - a context owns one stream, one workspace and one program cache, all
 *     per device; a mask would need per-device copies of each behind one
 *     handle and serialise the devices inside a call.
 * A mask maps onto this by calling mg_init once per set bit.  Every entry
 * point makes the context's device current (hipSetDevice) before it touches
 * device memory, so one thread may drive contexts on different devices.
 * MYTHGPU_LDS_SLOTS (LDS spill regions per lane; default: the layout's,
 * mg_layouts) must be an integer 0..MG_MAX_LDS_DS, else MG_E_ARG.
 *
 * Register layouts: the library holds one assembly
 * interpreter per layout — 16 slots at three waves per SIMD and 11 slots
 * (MG_NREG_W4) in 128 VGPRs at four — and a context runs ONE of them:
 * mg_init_layout(device, nreg) picks it (mg_init = the 16-slot layout).
 * Programs loaded into a context must be compiled for its slot count
 * (mg_load_program refuses a slot index >= nreg), so a caller chooses the
 * layout per batch by choosing the context it loads the batch into. */
int mg_init(int device, mg_ctx** out);
int mg_init_layout(int device, uint32_t nreg, mg_ctx** out);
/* The layouts this library holds (no GPU needed): out[3i..3i+2] = (slots,
 * waves per SIMD, default LDS spill regions) of layout i, for as many as n
 * words hold; returns the number of layouts. */
int mg_layouts(uint32_t* out, uint32_t n);
void mg_free(mg_ctx* ctx);
const char* mg_last_error(const mg_ctx* ctx);
/* Device time (ms, HIP events on the context stream) of the last synchronous
 * mg_eval / mg_eval_gen / mg_search / mg_batch_search: the evaluation or
 * search launches only (no copies, no witness regeneration).  Feeds
 * SolverStatistics' kernel time (reference solver_statistics.py:29-43). */
float mg_last_kernel_ms(const mg_ctx* ctx);
/* CU count, device name; available after mg_init. */
int mg_device_info(mg_ctx* ctx, char* name, size_t name_len, int* n_cus);

/* Upload one compiled program (IR of include/mythgpu_ir.h).  n_spill_slots
 * spill slots are used by SPILL/RELOAD; the first MG_MAX_LDS of them live in
 * LDS, the rest (<= MG_MAX_PSLOTS) in per-lane scratch. */
int mg_load_program(mg_ctx* ctx, const uint32_t* code, uint32_t n_ins,
                    const uint32_t* consts, uint32_t n_consts,
                    const mg_leafgen* leaves, uint32_t n_leaves,
                    uint32_t n_spill_slots, uint32_t n_probes, uint64_t prog_seed,
                    mg_prog** out);
void mg_free_program(mg_prog* prog);

/* Evaluate under caller assignments (host buffers).
 *   leaves_soa : [n_leaves][8][n_assign] u32 limbs, little-endian
 *   root_bits  : [ceil(n_assign/64)] u64, bit i = conjunction of ROOTs
 *   probes     : [n_probes][8][n_assign] u32, or NULL */
int mg_eval(mg_ctx* ctx, const mg_prog* prog, const uint32_t* leaves_soa, uint64_t n_assign,
            uint64_t* root_bits, uint32_t* probes);

/* Evaluate under device-generated assignments (candidate indices
 * gen->first_index ...).  leaves_out: [n_leaves][8][n_assign] or NULL. */
int mg_eval_gen(mg_ctx* ctx, const mg_prog* prog, const mg_gen* gen, uint64_t n_assign,
                uint64_t* root_bits, uint32_t* probes, uint32_t* leaves_out);

/* Witness search: smallest candidate index in [gen->first_index,
 * gen->first_index + n_cand) whose assignment satisfies every ROOT, or -1.
 * witness_leaves ([n_leaves][8], may be NULL) receives its leaf values.  The
 * whole range is queued on the device at once (no host round trip per
 * chunk); waves beyond the first witness found so far exit immediately. */
int mg_search(mg_ctx* ctx, const mg_prog* prog, const mg_gen* gen, uint64_t n_cand,
              int64_t* first_sat, uint32_t* witness_leaves);

/* Verdict census: over the candidates [gen->first_index, gen->first_index +
 * n_cand), per constraint ("root") k of the program, how the search failed.
 * No reference counterpart: it serves the misses of Constraints.is_possible
 * (reference laser/ethereum/state/constraints.py:26-45), which reports only
 * that no model was found.
 * The program carries its verdict mask as probes mask_probe0 ..
 * mask_probe0 + ceil(n_roots / 256) - 1: bit k % 256 of probe mask_probe0 +
 * k / 256 = root k holds (mythril_amd/census.py mask_probes; bits at or
 * above n_roots are ignored).  Per chunk of `chunk` candidates (0: 2^16;
 * else a multiple of 256) the interpreter launch and the census kernel
 * (mg_census.hip) are queued on the context stream; the counters stay on the
 * device until one copy at the end.  Outputs (n_roots entries unless noted):
 *   pass[k]        candidates on which root k holds
 *   first_block[k] candidates whose lowest failing root is k
 *   sole_block[k]  candidates on which root k is the only failing root
 *   sole_index[k]  the smallest such candidate index, or -1
 *   nfail_hist[f]  f = 0..n_roots (n_roots + 1 entries): candidates with
 *                  exactly f failing roots
 *   best_nfail, best_index   the minimum of (failing roots, candidate index)
 *                  in lexicographic order; n_roots + 1 and -1 when n_cand = 0
 * Sums and minima only: identical across runs and chunk sizes.  MG_E_ARG
 * without a launch for: a null pointer, n_roots outside 1..1024, mask probes
 * outside the program's probes, a chunk that is not a multiple of 256, a
 * first_index that is not a multiple of 64 (the generator's class groups),
 * 2^53 candidates or more, and a program whose probes need more than 256 MiB
 * per chunk (load the census view, which writes the mask probes only).
 * mg_last_kernel_ms covers the launches. */
int mg_census(mg_ctx* ctx, const mg_prog* prog, const mg_gen* gen, uint64_t n_cand,
              uint32_t n_roots, uint32_t mask_probe0, uint64_t chunk, uint64_t* pass,
              uint64_t* first_block, uint64_t* sole_block, int64_t* sole_index,
              uint64_t* nfail_hist, uint32_t* best_nfail, int64_t* best_index);

/* The censuses of several programs over one candidate range in one launch
 * sequence (csrc/mg_census_batch.h, mg_census_batch.hip).
 * Like mg_census it serves the misses of Constraints.is_possible (reference
 * laser/ethereum/state/constraints.py:26-45): a query that misses in several
 * independent groups asks for one census per group.  jobs[k] names a program
 * that carries its verdict mask as mg_census describes; all jobs share gen
 * (seed and first_index), as the programs of mg_batch_search do.  Per chunk,
 * one interpreter launch over all jobs and one launch of
 * mg_census_batch_kernel; the counters of all jobs are preset by one upload
 * and read by one copy.  Outputs: the seven outputs of mg_census for job k at
 * pass + k * max_roots, first_block + k * max_roots, sole_block + k *
 * max_roots, sole_index + k * max_roots, nfail_hist + k * (max_roots + 1),
 * best_nfail[k] and best_index[k], each with mg_census's conventions and bit
 * for bit what mg_census returns for job k alone; entries past a job's n_roots
 * are zero (-1 in sole_index).  chunk 0: the largest multiple of 256, at most
 * 2^16, at which the probe regions of all jobs fit 256 MiB.
 * Refused with MG_E_ARG before any upload or launch, the message beginning
 * "census_batch:": a null pointer; n_jobs outside 1..MG_CENSUS_BATCH_MAX_JOBS;
 * a program of another context; a chunk that is not a multiple of 256, a
 * first_index that is not a multiple of 64, 2^53 candidates or more; an
 * explicit chunk whose probe regions exceed 256 MiB (the message gives the
 * bytes needed), and jobs whose regions exceed it at 256 lanes (load the
 * census view, or pass fewer jobs); and, as "census_batch: job k: ...", a
 * job's n_roots above max_roots and whatever mg_census refuses for job k.
 * n_cand = 0: empty censuses and no launch.  mg_last_kernel_ms covers the
 * launches. */
typedef struct mg_census_job {
    const mg_prog* prog;
    uint32_t n_roots, mask_probe0;
} mg_census_job;
/* The counts of one job that size its share of the batch's device buffer. */
typedef struct mg_census_shape {
    uint32_t n_probes;                /* of the job's program */
    uint32_t n_roots, mask_probe0;
} mg_census_shape;
/* The cap of mg_walk_batch: the grid's y dimension allows 65535, and 256
 * counter blocks of 1024 roots are about 10 MB to preset and to read. */
#define MG_CENSUS_BATCH_MAX_JOBS 256u
int mg_census_batch(mg_ctx* ctx, const mg_census_job* jobs, uint32_t n_jobs, const mg_gen* gen,
                    uint64_t n_cand, uint64_t chunk, uint32_t max_roots, uint64_t* pass,
                    uint64_t* first_block, uint64_t* sole_block, int64_t* sole_index,
                    uint64_t* nfail_hist, uint32_t* best_nfail, int64_t* best_index);
/* Host-only (no GPU): the plan of the device buffer mg_census_batch uses
 * (csrc/mg_census_batch.h says what lies where).  out_offsets:
 * [MG_CENSUS_BATCH_SHARED + n_jobs * MG_CENSUS_BATCH_JOB_REGIONS] byte
 * offsets: the descriptors, the job records, then job by job its counter
 * block and its probe region.  In address order — descriptors, records, all
 * counter blocks, all probe regions — every region is 256-byte aligned and
 * ends where the next begins, the last at *out_bytes.  *out_chunk: the
 * candidates per launch (`chunk`, or what chunk 0 chooses).  MG_E_ARG for a
 * null pointer, n_jobs outside 1..MG_CENSUS_BATCH_MAX_JOBS, a chunk that is
 * no multiple of 256 or whose probe regions exceed 256 MiB, jobs that do not
 * fit at 256 lanes, and sizes beyond 64 bits; `why` (may be NULL; why_len
 * bytes) then receives the refusal as mg_census_batch words it, after the
 * "census_batch: ". */
#define MG_CENSUS_BATCH_SHARED 2
#define MG_CENSUS_BATCH_JOB_REGIONS 2
int mg_census_batch_plan_host(const mg_census_shape* shapes, uint32_t n_jobs, uint64_t n_cand,
                              uint64_t chunk, uint64_t* out_offsets, uint64_t* out_bytes,
                              uint64_t* out_chunk, char* why, size_t why_len);
/* Host-only (no GPU): blocks per job of one mg_census_batch_kernel launch over
 * n candidates: min(ceil(n / 256), max(1, 2048 / n_jobs)); tiles beyond are
 * grid-strided.  0 for n_jobs = 0 or n = 0. */
int mg_census_batch_blocks_host(uint32_t n_jobs, uint64_t n);

/* Local search from a nearly satisfying assignment, e.g.
 * the census's best candidate.  No reference counterpart: like the census it
 * serves the misses of Constraints.is_possible (reference
 * laser/ethereum/state/constraints.py:26-45), where the candidate stream
 * keeps landing one or two constraints short of a model and every candidate
 * is a fresh draw.
 * The program carries its verdict mask as probes mask_probe0 .. (as for
 * mg_census).  Per round, on the context stream and with no host round trip:
 * `lanes` neighbours of the base assignment are written on the device (lane 0
 * is the base, the lower half differs from it by one move, the upper half by
 * two; csrc/mg_repair.h is the move function, mythril_amd/repair.py its
 * specification), the interpreter evaluates their verdict masks in eval
 * mode, and the neighbour with the fewest failing roots (ties: the lowest
 * lane) becomes the base when it fails strictly fewer than the base does.
 * After every sync_every rounds (0: 8) the host reads the base's failing
 * count and stops at 0 or after max_rounds.  Outputs:
 *   out_leaves [n_leaves][8]  the last base
 *   out_nfail                 its failing roots (0: it satisfies every root)
 *   out_rounds                rounds run
 *   trace [max_rounds] or NULL: the fewest failing roots of each round run
 *                             (0 beyond out_rounds)
 * A function of the arguments alone: identical across runs.  MG_E_ARG without
 * a launch for: a null pointer other than trace, a program with no leaves,
 * n_roots outside 1..1024, mask probes outside the program's probes, lanes
 * outside 1..2^20, max_rounds outside 1..2^16, and a program whose probes
 * need more than 256 MiB (load the census view).  mg_last_kernel_ms covers
 * the rounds. */
int mg_repair(mg_ctx* ctx, const mg_prog* prog, const uint32_t* start_leaves /*[n_leaves][8]*/,
              uint32_t n_roots, uint32_t mask_probe0, uint64_t seed, uint32_t lanes,
              uint32_t max_rounds, uint32_t sync_every,
              uint32_t* out_leaves /*[n_leaves][8]*/, uint32_t* out_nfail,
              uint32_t* out_rounds, uint32_t* trace /*[max_rounds] or NULL*/);
/* Host-only (no GPU): the neighbours mg_repair's round r writes for lanes
 * lane0 .. lane0 + n_lanes - 1 of `lanes`, from the same move function:
 * out [n_leaves][8][n_lanes]; moves ([n_lanes][4] or NULL): the number of
 * moves, kind of move 0 | kind of move 1 << 8, leaf of move 0, leaf of move
 * 1.  MG_E_ARG for a null pointer, no leaves, a width outside 1..256, a pool
 * outside the constants, a base value beyond its width, lanes outside
 * 1..2^20, r at or above 2^16 and a lane range outside lanes. */
int mg_repair_mutate_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                          uint32_t n_consts, const uint32_t* base /*[n_leaves][8]*/,
                          uint64_t seed, uint32_t r, uint32_t lanes, uint32_t lane0,
                          uint32_t n_lanes, uint32_t* out, uint32_t* moves);

/* Scored walk: `walkers` local searches in one launch
 * sequence, neighbours ranked by (failing roots, cost) instead of the failing
 * count alone.  Like mg_repair it has no reference counterpart and serves the
 * misses of Constraints.is_possible (reference
 * laser/ethereum/state/constraints.py:26-45).
 * The program carries its verdict mask as probes mask_probe0 .. (as for
 * mg_census) and, right after the mask, n_resid residual probes
 * (mythril_amd/repair.py residuals).  table[k] = kind << 16 | index of root
 * k's residual among them; a failing root costs its distance: kind 0 (flat)
 * 1, kind 1 (Hamming, residual a xor b of a root a = b) max(1, popcount),
 * kind 2 (magnitude, residual a - b of an order root) 1 + bit length.  cost =
 * the sum over the failing roots (csrc/mg_walk.h; repair.py score_ref is its
 * specification).  Whether a root holds is read from the mask alone.
 * Walker w starts at starts[w] and draws the moves of mg_repair under the
 * seed seed ^ w * MG_WALK_CW.  Per round, on the context stream and with no
 * host round trip, every walker's `lanes` neighbours are written, evaluated
 * in ONE eval-mode launch over walkers * lanes lanes and scored; a walker
 * adopts its best neighbour (ties: the lowest lane) on a strict improvement
 * of (failing roots, cost).  After every sync_every rounds (0: 8) the host
 * reads the walkers' states and stops once any walker has no failing root, or
 * after max_rounds.  Outputs:
 *   out_leaves [walkers][n_leaves][8]  each walker's last base
 *   out_nfail, out_cost [walkers]      its failing roots and cost
 *   out_rounds                         rounds run (the same for every walker)
 *   trace [walkers][max_rounds][2] or NULL: (failing roots, cost) of each
 *                                      walker's best neighbour per round run
 *                                      (0 beyond out_rounds)
 *   out_winner                         the walker of minimum (nfail, cost, w)
 * A function of the arguments alone: identical across runs.  MG_E_ARG without
 * a launch for: a null pointer other than trace, a program with no leaves,
 * walkers outside 1..64, n_roots outside 1..1024, mask or residual probes
 * outside the program's probes, lanes outside 1..2^20, max_rounds outside
 * 1..2^16, a table entry with an unknown kind or a residual index at or
 * above n_resid, and walkers * lanes * probes * 32 B above 256 MiB (load the
 * census view).  mg_last_kernel_ms covers the rounds. */
int mg_walk(mg_ctx* ctx, const mg_prog* prog, const uint32_t* starts /*[walkers][n_leaves][8]*/,
            uint32_t walkers, uint32_t n_roots, uint32_t mask_probe0,
            const uint32_t* table /*[n_roots]*/, uint32_t n_resid, uint64_t seed, uint32_t lanes,
            uint32_t max_rounds, uint32_t sync_every,
            uint32_t* out_leaves /*[walkers][n_leaves][8]*/, uint32_t* out_nfail /*[walkers]*/,
            uint32_t* out_cost /*[walkers]*/, uint32_t* out_rounds,
            uint32_t* trace /*[walkers][max_rounds][2] or NULL*/, uint32_t* out_winner);
/* Host-only (no GPU): mg_walk's scoring function on n lanes.  masks:
 * [ceil(n_roots / 256) * 8][n] u32, the rows of the verdict mask; resid:
 * [n_resid * 8][n] u32 (may be NULL when n_resid = 0); nfail, cost: [n].
 * MG_E_ARG for a null pointer, n_roots outside 1..1024 and a table entry
 * mg_walk refuses. */
int mg_walk_score_host(const uint32_t* masks, const uint32_t* resid, const uint32_t* table,
                       uint32_t n_roots, uint32_t n_resid, uint64_t n, uint32_t* nfail,
                       uint32_t* cost);

/* Scored walk with tree distances: mg_walk, but a failing
 * root may cost the branch distance of a small postfix program over atoms
 * (and = sum, or = minimum), so a root made of equalities and orders under
 * and / or / ite / store chains has a gradient.  The program carries, from
 * probe mask_probe0 on: the root mask (ceil(n_roots / 256) probes), the atom
 * mask (ceil(n_atoms / 256) probes, bit i: atom i holds), then n_resid
 * residual probes.  roots[k] is a table entry of mg_walk or 1 << 31 | offset
 * of the root's program in code; atoms[i] = kind << 16 | residual probe;
 * code: words op << 16 | argument (csrc/mg_walk_tree.h fixes the encoding and
 * the limits; mythril_amd/repair.py distance_trees builds the tables,
 * tree_score_ref is the specification).  Moves, rounds, walkers, outputs and
 * workspace are those of mg_walk.  Refused without a launch: what mg_walk
 * refuses, n_atoms above 1024, atom-mask or residual probes outside the
 * program's probes, and tables mg_walk_tree_ok refuses (unknown kind or
 * opcode, atom or residual index out of range, offset outside code, a stack
 * that underflows or is deeper than 8, a program that does not end with one
 * value, more than 32 atoms or 64 words per root). */
int mg_walk_tree(mg_ctx* ctx, const mg_prog* prog,
                 const uint32_t* starts /*[walkers][n_leaves][8]*/, uint32_t walkers,
                 uint32_t n_roots, uint32_t mask_probe0, const uint32_t* roots /*[n_roots]*/,
                 uint32_t n_atoms, const uint32_t* atoms /*[n_atoms] or NULL*/,
                 const uint32_t* code /*[n_code] or NULL*/, uint32_t n_code, uint32_t n_resid,
                 uint64_t seed, uint32_t lanes, uint32_t max_rounds, uint32_t sync_every,
                 uint32_t* out_leaves /*[walkers][n_leaves][8]*/,
                 uint32_t* out_nfail /*[walkers]*/, uint32_t* out_cost /*[walkers]*/,
                 uint32_t* out_rounds, uint32_t* trace /*[walkers][max_rounds][2] or NULL*/,
                 uint32_t* out_winner);
/* Host-only (no GPU): mg_walk_tree's scoring function on n lanes.  masks,
 * amasks: the rows of the root mask and of the atom mask ([.. * 8][n] u32;
 * amasks may be NULL when n_atoms = 0), resid as for mg_walk_score_host.
 * MG_E_ARG for a null pointer and for tables mg_walk_tree refuses. */
int mg_walk_tree_score_host(const uint32_t* masks, const uint32_t* amasks, const uint32_t* resid,
                            const uint32_t* roots, uint32_t n_roots, const uint32_t* atoms,
                            uint32_t n_atoms, const uint32_t* code, uint32_t n_code,
                            uint32_t n_resid, uint64_t n, uint32_t* nfail, uint32_t* cost);

/* Tree-scored walk with aimed moves: mg_walk_tree, but some
 * lanes of a round apply a move aimed by a failing equality's residual.  A
 * HAMMING atom a = b carries the residual probe R = a xor b; where a side is
 * made of leaves, flipping in those leaves the bits set in R makes the atom
 * hold.  The aim table lists such sides (mythril_amd/repair.py aim_table
 * builds it, aim_mutate_ref is the specification, csrc/mg_walk_aim.h fixes
 * the lane layout):
 *   entries [n_entries][3]  residual probe, first piece, number of pieces
 *   pieces  [n_pieces][4]   leaf, leaf_bit, value_bit, len: the piece does
 *                           leaf ^= ((R >> value_bit) & (2^len - 1)) << leaf_bit
 * R is the entry's residual under the walker's current base: on adoption the
 * adopted lane's residual values are kept per walker, so aimed lanes exist
 * from round 1 on.  With L the entries whose R is not zero, in table order,
 * and n1 = min(|L|, lanes / 8): lanes 1 .. n1 are the base with entry
 * L[(j - 1 + r * n1) mod |L|] applied, lanes n1 + 1 .. 2 * n1 the same entry
 * for j - n1 with mg_repair's moves of lane j written over it, every other
 * lane is mg_repair's neighbour.  With no entry the walk is mg_walk_tree bit
 * for bit.  Scoring, rounds, walkers, outputs and workspace are those of
 * mg_walk_tree.  Refused without a launch: what mg_walk_tree refuses, and an
 * aim table mg_walk_aim_ok refuses (more than 256 entries, a residual index
 * at or above n_resid, an entry without pieces, with more than 64 or with
 * pieces outside the piece array, a leaf at or above n_leaves, leaf_bit + len
 * above the leaf's width, value_bit + len above 256). */
int mg_walk_aim(mg_ctx* ctx, const mg_prog* prog,
                const uint32_t* starts /*[walkers][n_leaves][8]*/, uint32_t walkers,
                uint32_t n_roots, uint32_t mask_probe0, const uint32_t* roots /*[n_roots]*/,
                uint32_t n_atoms, const uint32_t* atoms /*[n_atoms] or NULL*/,
                const uint32_t* code /*[n_code] or NULL*/, uint32_t n_code, uint32_t n_resid,
                const uint32_t* entries /*[n_entries][3] or NULL*/, uint32_t n_entries,
                const uint32_t* pieces /*[n_pieces][4] or NULL*/, uint32_t n_pieces,
                uint64_t seed, uint32_t lanes, uint32_t max_rounds, uint32_t sync_every,
                uint32_t* out_leaves /*[walkers][n_leaves][8]*/,
                uint32_t* out_nfail /*[walkers]*/, uint32_t* out_cost /*[walkers]*/,
                uint32_t* out_rounds, uint32_t* trace /*[walkers][max_rounds][2] or NULL*/,
                uint32_t* out_winner);
/* Host-only (no GPU): mg_repair_mutate_host for mg_walk_aim's lane function.
 * rvals: the residual values of the base ([n_resid][8]; NULL: round 0, no
 * residual known, every lane is mg_repair's); moves ([n_lanes][5] or NULL):
 * the four words of mg_repair_mutate_host (the number of moves is 0 where
 * mg_repair's moves do not apply), then the aimed entry or 0xFFFFFFFF.
 * MG_E_ARG for what mg_repair_mutate_host refuses and for an aim table
 * mg_walk_aim refuses. */
int mg_walk_aim_mutate_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                            uint32_t n_consts, const uint32_t* base /*[n_leaves][8]*/,
                            const uint32_t* rvals /*[n_resid][8] or NULL*/, uint32_t n_resid,
                            const uint32_t* entries, uint32_t n_entries, const uint32_t* pieces,
                            uint32_t n_pieces, uint64_t seed, uint32_t r, uint32_t lanes,
                            uint32_t lane0, uint32_t n_lanes, uint32_t* out, uint32_t* moves);

/* Tree-scored walk with moves aimed by equalities and orders (DESIGN.md
 * §3.13): mg_walk_aim with a wider aim table.  A MAGNITUDE atom lo < hi or
 * lo <= hi carries the residual probe D = lo - hi; where a side is made of
 * leaves, lo := lo - D - s or hi := hi + D + s (s = 1 for a strict order)
 * makes the atom hold (mythril_amd/repair.py bound_table builds the table,
 * bound_mutate_ref is the specification, csrc/mg_walk_bound.h the code):
 *   entries [n_entries][5]  residual probe, first piece, number of pieces,
 *                           mode (0 XOR, 1 LOW, 2 LOW_STRICT, 3 HIGH,
 *                           4 HIGH_STRICT), truth (1 << 31 | i: bit i of the
 *                           atom mask, else bit k of the root mask; 0 for XOR)
 *   pieces  [n_pieces][4]   as for mg_walk_aim
 *   fixed   [n_entries][8]  the numeral bits of an order entry's side (0 for XOR)
 * An XOR entry acts and is live as in mg_walk_aim.  An order entry is live
 * iff its truth bit is clear on the walker's base (the adopted lane's mask
 * rows are kept per walker); it gathers V = fixed | the pieces' bits of the
 * base, takes T = V - D - s (LOW) or V + D + s (HIGH) mod 2^256 and writes
 * T's bits back through the pieces.  Lane layout, scoring, rounds, walkers,
 * outputs and workspace are those of mg_walk_aim; with XOR entries only the
 * walk is mg_walk_aim bit for bit.  Refused without a launch: what
 * mg_walk_aim refuses, a mode above 4, a truth index at or above n_atoms
 * (n_roots), an XOR entry with a truth or fixed word set, and a null table
 * with a non-zero count. */
int mg_walk_bound(mg_ctx* ctx, const mg_prog* prog,
                  const uint32_t* starts /*[walkers][n_leaves][8]*/, uint32_t walkers,
                  uint32_t n_roots, uint32_t mask_probe0, const uint32_t* roots /*[n_roots]*/,
                  uint32_t n_atoms, const uint32_t* atoms /*[n_atoms] or NULL*/,
                  const uint32_t* code /*[n_code] or NULL*/, uint32_t n_code, uint32_t n_resid,
                  const uint32_t* entries /*[n_entries][5] or NULL*/, uint32_t n_entries,
                  const uint32_t* pieces /*[n_pieces][4] or NULL*/, uint32_t n_pieces,
                  const uint32_t* fixed /*[n_entries][8] or NULL*/,
                  uint64_t seed, uint32_t lanes, uint32_t max_rounds, uint32_t sync_every,
                  uint32_t* out_leaves /*[walkers][n_leaves][8]*/,
                  uint32_t* out_nfail /*[walkers]*/, uint32_t* out_cost /*[walkers]*/,
                  uint32_t* out_rounds, uint32_t* trace /*[walkers][max_rounds][2] or NULL*/,
                  uint32_t* out_winner);
/* Host-only (no GPU): mg_walk_aim_mutate_host for mg_walk_bound's lane
 * function.  rvals: the base's residual values, mvals: its mask state, the
 * root-mask words ([ceil(n_roots / 256) * 8]) then the atom-mask words
 * ([ceil(n_atoms / 256) * 8]); either NULL: round 0, every lane is
 * mg_repair's.  MG_E_ARG for what mg_walk_aim_mutate_host refuses and for a
 * table mg_walk_bound refuses. */
int mg_walk_bound_mutate_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                              uint32_t n_consts, const uint32_t* base /*[n_leaves][8]*/,
                              const uint32_t* rvals /*[n_resid][8] or NULL*/, uint32_t n_resid,
                              const uint32_t* mvals, uint32_t n_roots, uint32_t n_atoms,
                              const uint32_t* entries, uint32_t n_entries, const uint32_t* pieces,
                              uint32_t n_pieces, const uint32_t* fixed, uint64_t seed, uint32_t r,
                              uint32_t lanes, uint32_t lane0, uint32_t n_lanes, uint32_t* out,
                              uint32_t* moves);

/* Tree-scored walk with aims that write the table entry a UF application
 * reads: mg_walk_bound whose pieces may name a UF slot,
 * 1 << 31 | u, instead of a leaf.  Slot u is one application; the leaf its
 * pieces act on is resolved per walker at every adoption from the adopted
 * base and the adopted lane's n_urows U rows — the probes after the residual
 * probes: the arguments' 256-bit chunks, then the computed keys of
 * argument-keyed entries (mythril_amd/repair.py uf_table builds the tables,
 * uf_resolve_ref and uf_mutate_ref are the specification, csrc/mg_walk_uf.h
 * the code):
 *   slots [n_slots][2]  function, first U row of the argument
 *   funcs [n_funcs][3]  first candidate, candidates, key chunks (1 .. 4)
 *   cands [n_cands][6]  value leaf or 0xFFFFFFFF, key kind (0 CONST: a row of
 *                       ukeys, 1 LEAF: a leaf, 2 PROBE: a U row, 3 ALWAYS),
 *                       one key word per chunk
 *   ukeys [n_ukeys][8]  the chunks of the constant keys
 * The destination of a slot is the value leaf of the first candidate of its
 * function whose key equals the argument; an entry with a slot piece that has
 * none is not live.  With no slot piece the walk is mg_walk_bound bit for
 * bit.  Refused without a launch: what mg_walk_bound refuses for leaf pieces;
 * more than 64 slots, 64 functions, 256 candidates or 128 U rows; a slot,
 * function, candidate, key or U-row index out of range; chunks outside
 * 1 .. 4; value leaves of one function of different widths; a slot piece
 * outside that width; U rows the program does not have; a null table with a
 * non-zero count. */
int mg_walk_uf(mg_ctx* ctx, const mg_prog* prog,
               const uint32_t* starts /*[walkers][n_leaves][8]*/, uint32_t walkers,
               uint32_t n_roots, uint32_t mask_probe0, const uint32_t* roots /*[n_roots]*/,
               uint32_t n_atoms, const uint32_t* atoms /*[n_atoms] or NULL*/,
               const uint32_t* code /*[n_code] or NULL*/, uint32_t n_code, uint32_t n_resid,
               const uint32_t* entries /*[n_entries][5] or NULL*/, uint32_t n_entries,
               const uint32_t* pieces /*[n_pieces][4] or NULL*/, uint32_t n_pieces,
               const uint32_t* fixed /*[n_entries][8] or NULL*/,
               const uint32_t* slots, uint32_t n_slots, const uint32_t* funcs, uint32_t n_funcs,
               const uint32_t* cands, uint32_t n_cands, const uint32_t* ukeys, uint32_t n_ukeys,
               uint32_t n_urows, uint64_t seed, uint32_t lanes, uint32_t max_rounds,
               uint32_t sync_every, uint32_t* out_leaves /*[walkers][n_leaves][8]*/,
               uint32_t* out_nfail /*[walkers]*/, uint32_t* out_cost /*[walkers]*/,
               uint32_t* out_rounds, uint32_t* trace /*[walkers][max_rounds][2] or NULL*/,
               uint32_t* out_winner);
/* Host-only (no GPU): the destinations of the slots under base and the U rows
 * urows, as the adopt kernel of mg_walk_uf resolves them; MG_E_ARG for tables
 * mg_walk_uf refuses. */
int mg_walk_uf_resolve_host(const mg_leafgen* leaves, uint32_t n_leaves,
                            const uint32_t* base /*[n_leaves][8]*/,
                            const uint32_t* urows /*[n_urows][8]*/, uint32_t n_urows,
                            const uint32_t* slots, uint32_t n_slots, const uint32_t* funcs,
                            uint32_t n_funcs, const uint32_t* cands, uint32_t n_cands,
                            const uint32_t* ukeys, uint32_t n_ukeys, uint32_t* dest /*[n_slots]*/);
/* Host-only (no GPU): mg_walk_bound_mutate_host for mg_walk_uf's lane
 * function; dest: the slots' destinations under the base. */
int mg_walk_uf_mutate_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                           uint32_t n_consts, const uint32_t* base /*[n_leaves][8]*/,
                           const uint32_t* rvals /*[n_resid][8] or NULL*/, uint32_t n_resid,
                           const uint32_t* mvals, uint32_t n_roots, uint32_t n_atoms,
                           const uint32_t* entries, uint32_t n_entries, const uint32_t* pieces,
                           uint32_t n_pieces, const uint32_t* fixed, const uint32_t* slots,
                           uint32_t n_slots, const uint32_t* funcs, uint32_t n_funcs,
                           const uint32_t* cands, uint32_t n_cands, const uint32_t* ukeys,
                           uint32_t n_ukeys, uint32_t n_urows, const uint32_t* dest /*[n_slots]*/,
                           uint64_t seed, uint32_t r, uint32_t lanes, uint32_t lane0,
                           uint32_t n_lanes, uint32_t* out, uint32_t* moves);

/* Tree-scored walk with aims through sums, differences, masks and shifts
 * (DESIGN.md §3.15): mg_walk_uf whose entries may be linear.  A linear entry
 * belongs to a side that is a sum of +-terms; its pieces and fixed value are
 * those of one term of the sum, the target, and its move changes the target
 * by what the side must change by (csrc/mg_walk_sum.h; mythril_amd/repair.py
 * sum_table builds the tables, sum_mutate_ref is the specification):
 *   lin [n_entries]  0: the entry is mg_walk_uf's.  Else bit 0 set; bit 1: the
 *                    target's sign in the side is -1; bits 8-15: the side row
 *                    (XOR mode; 0 in the order modes); every other bit 0
 * The program writes n_srows side rows (at most 64), one 256-bit probe per
 * linear side with an XOR entry, after the n_resid residual probes and before
 * the n_urows U rows.  With lin all 0 the walk is mg_walk_uf bit for bit.
 * Refused without a launch: what mg_walk_uf refuses (a linear XOR entry may
 * have fixed bits); an unknown lin word; a side row at or above n_srows, or
 * one in a linear order entry; a slot piece in a linear entry; side rows and
 * U rows the program does not have; a null table with a non-zero count. */
int mg_walk_sum(mg_ctx* ctx, const mg_prog* prog,
                const uint32_t* starts /*[walkers][n_leaves][8]*/, uint32_t walkers,
                uint32_t n_roots, uint32_t mask_probe0, const uint32_t* roots /*[n_roots]*/,
                uint32_t n_atoms, const uint32_t* atoms /*[n_atoms] or NULL*/,
                const uint32_t* code /*[n_code] or NULL*/, uint32_t n_code, uint32_t n_resid,
                const uint32_t* entries /*[n_entries][5] or NULL*/, uint32_t n_entries,
                const uint32_t* pieces /*[n_pieces][4] or NULL*/, uint32_t n_pieces,
                const uint32_t* fixed /*[n_entries][8] or NULL*/,
                const uint32_t* lin /*[n_entries] or NULL*/, uint32_t n_srows,
                const uint32_t* slots, uint32_t n_slots, const uint32_t* funcs, uint32_t n_funcs,
                const uint32_t* cands, uint32_t n_cands, const uint32_t* ukeys, uint32_t n_ukeys,
                uint32_t n_urows, uint64_t seed, uint32_t lanes, uint32_t max_rounds,
                uint32_t sync_every, uint32_t* out_leaves /*[walkers][n_leaves][8]*/,
                uint32_t* out_nfail /*[walkers]*/, uint32_t* out_cost /*[walkers]*/,
                uint32_t* out_rounds, uint32_t* trace /*[walkers][max_rounds][2] or NULL*/,
                uint32_t* out_winner);
/* Host-only (no GPU): mg_walk_uf_mutate_host for mg_walk_sum's lane function;
 * svals: the side rows of the base. */
int mg_walk_sum_mutate_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                            uint32_t n_consts, const uint32_t* base /*[n_leaves][8]*/,
                            const uint32_t* rvals /*[n_resid][8] or NULL*/, uint32_t n_resid,
                            const uint32_t* mvals, uint32_t n_roots, uint32_t n_atoms,
                            const uint32_t* entries, uint32_t n_entries, const uint32_t* pieces,
                            uint32_t n_pieces, const uint32_t* fixed, const uint32_t* lin,
                            const uint32_t* svals /*[n_srows][8] or NULL*/, uint32_t n_srows,
                            const uint32_t* slots, uint32_t n_slots, const uint32_t* funcs,
                            uint32_t n_funcs, const uint32_t* cands, uint32_t n_cands,
                            const uint32_t* ukeys, uint32_t n_ukeys, uint32_t n_urows,
                            const uint32_t* dest /*[n_slots]*/, uint64_t seed, uint32_t r,
                            uint32_t lanes, uint32_t lane0, uint32_t n_lanes, uint32_t* out,
                            uint32_t* moves);

/* The walks of several groups in one launch sequence.  A
 * job is what mg_walk_sum takes for one program; walkers, lanes, max_rounds
 * and sync_every are shared by the batch, and the same mg_prog may appear in
 * several jobs.  Every output of job g (leaves, nfail, cost, rounds, winner,
 * trace) is byte for byte what mg_walk_sum returns for job g alone with the
 * same shared arguments — and with empty tables what mg_walk_uf, _bound, _aim
 * and _tree return, as mg_walk_sum documents.  A round of the batch is four
 * launches, each n_jobs times as wide as the single walk's; after every
 * sync_every rounds the host reads all states, and a job one of whose walkers
 * has no failing root is frozen there, as its single walk would have stopped:
 * its rounds are fixed, no kernel works on it again and its trace rows past
 * the stop stay zero.  The batch ends when every job is frozen or after
 * max_rounds rounds. */
typedef struct mg_walk_job {
    const mg_prog* prog;
    const uint32_t* starts;           /* [walkers][n_leaves][8] */
    const uint32_t* roots;            /* [n_roots] */
    const uint32_t* atoms;            /* [n_atoms] or NULL */
    const uint32_t* code;             /* [n_code] or NULL */
    const uint32_t* entries;          /* [n_entries][5] or NULL */
    const uint32_t* pieces;           /* [n_pieces][4] or NULL */
    const uint32_t* fixed;            /* [n_entries][8] or NULL */
    const uint32_t* lin;              /* [n_entries] or NULL */
    const uint32_t *slots, *funcs, *cands, *ukeys;
    uint32_t* out_leaves;             /* [walkers][n_leaves][8] */
    uint32_t* out_nfail;              /* [walkers] */
    uint32_t* out_cost;               /* [walkers] */
    uint32_t* out_rounds;
    uint32_t* trace;                  /* [walkers][max_rounds][2] or NULL */
    uint32_t* out_winner;
    uint64_t seed;
    uint32_t n_roots, mask_probe0, n_atoms, n_code, n_resid, n_entries, n_pieces, n_srows,
             n_slots, n_funcs, n_cands, n_ukeys, n_urows;
} mg_walk_job;
/* The counts of one job that size its share of the batch's device buffer. */
typedef struct mg_walk_shape {
    uint32_t n_leaves, n_probes;      /* of the job's program */
    uint32_t n_roots, mask_probe0, n_atoms, n_code, n_resid, n_entries, n_pieces, n_srows,
             n_slots, n_funcs, n_cands, n_ukeys, n_urows;
} mg_walk_shape;
/* Jobs of one batch.  A job of one walker at 4096 lanes is 16 blocks, so 16
 * jobs fill the device's 256 CUs once and 256 jobs sixteen times over: past
 * that a wider grid gains nothing, while the states the host reads at every
 * sync point (16 bytes per walker and job) and the buffer grow with it.  Far
 * below the 65535 a grid's z dimension allows; callers with more jobs run
 * several batches (mythril_amd/engine.py walk_batch does). */
#define MG_WALK_BATCH_MAX_JOBS 256u
/* max_bytes 0: the batch's device buffer may take this much (1 GiB) */
#define MG_WALK_BATCH_DEFAULT_BYTES ((uint64_t)1 << 30)
/* Refused with MG_E_ARG before any upload or launch, the message beginning
 * "walk_batch:": n_jobs outside 1..MG_WALK_BATCH_MAX_JOBS; walkers, lanes or
 * max_rounds outside mg_walk_sum's ranges; a null job array, program or
 * output pointer; a program of another context; a buffer above max_bytes
 * (the message gives the bytes needed); and, as "walk_batch: job k: ...",
 * whatever mg_walk_sum refuses for job k. */
int mg_walk_batch(mg_ctx* ctx, const mg_walk_job* jobs, uint32_t n_jobs, uint32_t walkers,
                  uint32_t lanes, uint32_t max_rounds, uint32_t sync_every, uint64_t max_bytes);
/* Host-only (no GPU): the plan of the device buffer mg_walk_batch uses
 * (csrc/mg_walk_batch.h says what lies where).  out_offsets:
 * [MG_WALK_BATCH_SHARED + n_jobs * MG_WALK_BATCH_JOB_REGIONS] byte offsets,
 * the shared regions (descriptors, jobs, frozen words, states, root bits) and
 * then job by job its 22 regions, the last two its leaf and its probe region;
 * every region is 256-byte aligned and ends where the next one in address
 * order begins, the last at *out_bytes.  MG_E_ARG: shared arguments out of
 * range, a null pointer, or a size beyond 64 bits. */
#define MG_WALK_BATCH_SHARED 5
#define MG_WALK_BATCH_JOB_REGIONS 22
int mg_walk_batch_plan_host(const mg_walk_shape* shapes, uint32_t n_jobs, uint32_t walkers,
                            uint32_t lanes, uint32_t max_rounds, uint64_t* out_offsets,
                            uint64_t* out_bytes);
/* Host-only (no GPU): 1 when the counts of a job are in the ranges
 * mg_walk_sum accepts (what it checks before it reads a table), else 0. */
int mg_walk_batch_shape_ok_host(const mg_walk_shape* shape);

/* Witness carry (csrc/mg_carry.h, mg_carry.hip): remembered
 * witnesses evaluated on the programs of the groups that extend them.  It
 * serves the path queries of Constraints.is_possible (reference
 * laser/ethereum/state/constraints.py:26-45): at a JUMPI the parent's model
 * satisfies one of the two children, and one evaluation confirms which.
 * A job names an eval-form program (loaded with its leaf generators), pin rows
 * and a pin mask.  Lane i of job j evaluates the candidate whose pinned leaves
 * (bit l % 32 of pin_mask[l / 32]) are the pin rows and whose free leaf l is
 * generator v9's value (above mg_leafgen) for (gen->seed, the program's
 * prog_seed, l, gen->first_index + i), the leaf's mg_leafgen and the program's
 * constant pool; every value is masked to the leaf's width, upper limbs zero.
 * first[j]: the lowest lane of 0 .. lanes - 1 on which every root of job j
 * holds, or -1; leaves[j]: that lane's leaf rows, zero where there is none and
 * past the program's leaves.  fill_out (may be NULL): the jobs' leaf regions
 * as the fill kernel wrote them, [n_jobs][leaf_stride_w] words with job j's
 * [n_leaves][8][lanes] at the front (mg_carry_plan_host gives the stride).
 * One call is a fixed sequence whatever n_jobs: one upload (descriptors, jobs,
 * masks, rows, generator tables), the fill launch, one eval-mode interpreter
 * launch over the job axis, the gather launch, one download.
 * mg_last_kernel_ms covers the three launches.
 * Refused with MG_E_ARG before any upload or launch, the message beginning
 * "carry_batch:": a null pointer (fill_out excepted); n_jobs outside
 * 1..MG_CARRY_MAX_JOBS; lanes outside 1..2^20; max_leaves above 2^20; a
 * program of another context; a program with more leaves than max_leaves; a
 * device buffer above 1 GiB (the message gives the bytes needed). */
typedef struct mg_carry_job {
    const mg_prog* prog;        /* eval-form program, loaded with its leaf generators */
    const uint32_t* pin_rows;   /* [n_leaves][8]; rows of free leaves ignored          */
    const uint32_t* pin_mask;   /* [(n_leaves + 31) / 32], bit l: leaf l is pinned     */
} mg_carry_job;
/* as the census batch: the grid's job dimension allows 65535, callers with
 * more jobs run several batches (mythril_amd/engine.py carry_batch does) */
#define MG_CARRY_MAX_JOBS 256u
#define MG_CARRY_MAX_LEAVES (1u << 20)
int mg_carry_batch(mg_ctx* ctx, const mg_carry_job* jobs, uint32_t n_jobs, const mg_gen* gen,
                   uint32_t lanes, int64_t* first /*[n_jobs], -1: none*/,
                   uint32_t* leaves /*[n_jobs][max_leaves][8]*/, uint32_t max_leaves,
                   uint32_t* fill_out /*NULL, or every job's leaf region copied back*/);
/* Host-only (no GPU): lanes lane0 .. lane0 + n_lanes - 1 of one job as the fill
 * kernel writes them, from the same lane function: out [n_leaves][8][n_lanes].
 * classes ([n_leaves][n_lanes] or NULL): the generator branch a free leaf took
 * (0 r0, 1 boundary, 2 pool, 3 uniform), 0xFFFFFFFF for a pinned leaf.
 * MG_E_ARG for a null pointer (consts may be NULL when n_consts is 0), a width
 * outside 1..256, a pool outside the constants, lanes outside 1..2^20 and a
 * lane range outside lanes. */
int mg_carry_fill_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                       uint32_t n_consts, uint64_t prog_seed,
                       const uint32_t* pin_rows /*[n_leaves][8]*/,
                       const uint32_t* pin_mask /*[(n_leaves + 31) / 32]*/, uint64_t seed,
                       uint64_t first_index, uint32_t lanes, uint32_t lane0, uint32_t n_lanes,
                       uint32_t* out, uint32_t* classes);
/* Host-only (no GPU): the plan of the device buffer mg_carry_batch uses
 * (csrc/mg_carry.h says what lies where).  out_offsets: [MG_CARRY_SHARED +
 * n_jobs * MG_CARRY_JOB_REGIONS] byte offsets: descriptors, job records, first
 * words, the output block; then job by job its mask, rows, generators and leaf
 * region.  In address order — descriptors, records, first words, every job's
 * mask, rows and generators, the output block, all leaf regions — every region
 * is 256-byte aligned and ends where the next begins, the last at *out_bytes.
 * *out_leaf_stride_w: words between two jobs' leaf regions, the batch's
 * largest n_leaves x 8 x lanes rounded up to 256 bytes.  MG_E_ARG for a null
 * pointer, n_jobs or lanes out of range and sizes beyond 64 bits. */
#define MG_CARRY_SHARED 4
#define MG_CARRY_JOB_REGIONS 4
int mg_carry_plan_host(const uint32_t* n_leaves /*[n_jobs]*/, uint32_t n_jobs, uint32_t lanes,
                       uint32_t max_leaves, uint64_t* out_offsets, uint64_t* out_bytes,
                       uint64_t* out_leaf_stride_w);

/* The pin ladder of the witness carry (csrc/mg_carry.h,
 * mg_carry_ladder.hip): several pin sets of a job tried in one launch
 * sequence.  A job names an eval-form program (loaded with its leaf
 * generators), ONE set of pin rows and n_rungs pin masks, strictest first,
 * mask r at pin_masks + r * ((n_leaves + 31) / 32).  A call has `lanes`
 * candidates per rung; with R the batch's largest n_rungs every job has
 * C = R x lanes columns.  Column c of job j lies on rung
 * r = min(c / lanes, n_rungs - 1) and holds candidate i = c % lanes: leaf l is
 * the pin row where bit l of mask r is set, else generator v9's value for
 * (gen->seed, the program's prog_seed, l, gen->first_index + i), every value
 * masked to the leaf's width — what lane i of mg_carry_batch holds under mask
 * r.  Every rung so replays the same candidates, and a job with fewer rungs
 * than R repeats its last one in the surplus columns.
 * first[j]: the lowest column of 0 .. C - 1 on which every root of job j
 * holds, or -1; rung[j]: that column's rung, or -1 — the strictest rung with
 * a hit, since rungs lie in column order; leaves[j]: that column's leaf rows,
 * zero where there is none and past the program's leaves.  fill_out (may be
 * NULL): the jobs' leaf regions as the fill kernel wrote them,
 * [n_jobs][leaf_stride_w] words with job j's [n_leaves][8][C] at the front
 * (mg_carry_ladder_plan_host gives the stride).
 * The sequence is mg_carry_batch's: one upload, the rung fill launch, one
 * eval-mode interpreter launch over the job axis at C candidates, the gather
 * launch, one download; mg_last_kernel_ms covers the three launches.  With
 * one rung per job the results are those of mg_carry_batch under that mask.
 * Refused with MG_E_ARG before any upload or launch, the message beginning
 * "carry_ladder:": whatever mg_carry_batch refuses; n_rungs outside
 * 1..MG_CARRY_MAX_RUNGS; R x lanes above 2^20; a null mask pointer. */
#define MG_CARRY_MAX_RUNGS 8u
typedef struct mg_carry_ladder_job {
    const mg_prog* prog;        /* eval-form program, loaded with its leaf generators */
    const uint32_t* pin_rows;   /* [n_leaves][8]; rows of leaves no rung pins ignored  */
    const uint32_t* pin_masks;  /* [n_rungs][(n_leaves + 31) / 32], strictest first    */
    uint32_t n_rungs;           /* 1..MG_CARRY_MAX_RUNGS                               */
    uint32_t pad;
} mg_carry_ladder_job;
int mg_carry_ladder(mg_ctx* ctx, const mg_carry_ladder_job* jobs, uint32_t n_jobs,
                    const mg_gen* gen, uint32_t lanes, int64_t* first /*[n_jobs], -1: none*/,
                    int64_t* rung /*[n_jobs], -1: none*/,
                    uint32_t* leaves /*[n_jobs][max_leaves][8]*/, uint32_t max_leaves,
                    uint32_t* fill_out /*NULL, or every job's leaf region copied back*/);
/* Host-only (no GPU): columns col0 .. col0 + n_cols - 1 of one job of
 * mg_carry_ladder as the rung fill kernel writes them, from the same lane
 * function: out [n_leaves][8][n_cols].  cols: the columns of the job, a
 * multiple of lanes in the call (n_rungs x lanes or more: the surplus repeats
 * the last rung).  MG_E_ARG as mg_carry_fill_host, and for n_rungs outside
 * 1..MG_CARRY_MAX_RUNGS, cols below lanes or above 2^20 and a column range
 * outside cols. */
int mg_carry_fill_rungs_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                             uint32_t n_consts, uint64_t prog_seed,
                             const uint32_t* pin_rows /*[n_leaves][8]*/,
                             const uint32_t* pin_masks /*[n_rungs][(n_leaves + 31) / 32]*/,
                             uint32_t n_rungs, uint64_t seed, uint64_t first_index,
                             uint32_t lanes, uint32_t cols, uint32_t col0, uint32_t n_cols,
                             uint32_t* out);
/* Host-only (no GPU): the plan of the device buffer mg_carry_ladder uses: the
 * regions of mg_carry_plan_host in the same order and under the same indices,
 * job j's mask region holding its n_rungs[j] masks, the output block first,
 * rung and rows, and every leaf region the batch's largest n_leaves x 8 x C
 * words rounded up to 256 bytes (*out_leaf_stride_w).  MG_E_ARG for a null
 * pointer, n_jobs, lanes or an n_rungs out of range, R x lanes above 2^20 and
 * sizes beyond 64 bits. */
int mg_carry_ladder_plan_host(const uint32_t* n_leaves /*[n_jobs]*/,
                              const uint32_t* n_rungs /*[n_jobs]*/, uint32_t n_jobs,
                              uint32_t lanes, uint32_t max_leaves, uint64_t* out_offsets,
                              uint64_t* out_bytes, uint64_t* out_leaf_stride_w);

/* Witness sets on the pin ladder (csrc/mg_carry.h,
 * mg_carry_sets.hip): a ladder whose rungs carry their own pin rows, so one
 * compiled group tries several remembered witnesses in one launch sequence.
 * A job names an eval-form program (loaded with its leaf generators), n_sets
 * sets of pin rows, set s at pin_rows + s * n_leaves * 8, n_rungs pin masks as
 * mg_carry_ladder_job has them, and rung_set: the row set of every rung.
 * The contract is mg_carry_ladder's word for word — the columns (C = R x
 * lanes, column c on rung r = min(c / lanes, n_rungs - 1) at candidate
 * c % lanes), first, rung, leaves, fill_out, the sequence (one upload, the set
 * fill launch, one eval-mode interpreter launch over the job axis at C
 * candidates, the gather launch of mg_carry_ladder, one download, no host
 * synchronisation inside) and what mg_last_kernel_ms covers — with ONE
 * difference: a leaf that mask r pins holds its row of set rung_set[r].  With
 * one set and rung_set all zero the results are those of mg_carry_ladder.
 * Refused with MG_E_ARG before any upload or launch, the message beginning
 * "carry_sets:": whatever mg_carry_ladder refuses; n_sets outside
 * 1..MG_CARRY_MAX_SETS; a null rung_set; a rung_set[r] not below n_sets. */
#define MG_CARRY_MAX_SETS 8u
typedef struct mg_carry_sets_job {
    const mg_prog* prog;        /* eval-form program, loaded with its leaf generators */
    const uint32_t* pin_rows;   /* [n_sets][n_leaves][8]                               */
    const uint32_t* pin_masks;  /* [n_rungs][(n_leaves + 31) / 32], strictest first    */
    const uint32_t* rung_set;   /* [n_rungs], each < n_sets                            */
    uint32_t n_rungs;           /* 1..MG_CARRY_MAX_RUNGS                               */
    uint32_t n_sets;            /* 1..MG_CARRY_MAX_SETS                                */
} mg_carry_sets_job;
int mg_carry_ladder_sets(mg_ctx* ctx, const mg_carry_sets_job* jobs, uint32_t n_jobs,
                         const mg_gen* gen, uint32_t lanes,
                         int64_t* first /*[n_jobs], -1: none*/,
                         int64_t* rung /*[n_jobs], -1: none*/,
                         uint32_t* leaves /*[n_jobs][max_leaves][8]*/, uint32_t max_leaves,
                         uint32_t* fill_out /*NULL, or every job's leaf region copied back*/);
/* Host-only (no GPU): mg_carry_fill_rungs_host for a job of
 * mg_carry_ladder_sets, from the set fill kernel's lane function.  MG_E_ARG as
 * mg_carry_fill_rungs_host, and for n_sets outside 1..MG_CARRY_MAX_SETS, a
 * null rung_set and a rung_set[r] not below n_sets. */
int mg_carry_fill_sets_host(const mg_leafgen* leaves, uint32_t n_leaves, const uint32_t* consts,
                            uint32_t n_consts, uint64_t prog_seed,
                            const uint32_t* pin_rows /*[n_sets][n_leaves][8]*/,
                            const uint32_t* pin_masks /*[n_rungs][(n_leaves + 31) / 32]*/,
                            const uint32_t* rung_set /*[n_rungs]*/, uint32_t n_rungs,
                            uint32_t n_sets, uint64_t seed, uint64_t first_index, uint32_t lanes,
                            uint32_t cols, uint32_t col0, uint32_t n_cols, uint32_t* out);
/* Host-only (no GPU): the plan of the device buffer mg_carry_ladder_sets uses.
 * out_offsets: mg_carry_ladder_plan_host's table — the same regions under the
 * same indices, job j's rows region holding its n_sets[j] row sets (n_sets[j]
 * x n_leaves[j] x 32 bytes) — followed by MG_CARRY_SETS_SHARED entries (the
 * set records) and MG_CARRY_SETS_JOB_REGIONS per job (its rung_set, n_rungs
 * u32).  In address order: descriptors, records, first words, every job's
 * masks, row sets and generators, the set records, every job's rung_set, the
 * output block, all leaf regions; every region 256-byte aligned.  MG_E_ARG
 * for what mg_carry_ladder_plan_host refuses, an n_sets outside
 * 1..MG_CARRY_MAX_SETS and sizes beyond 64 bits. */
#define MG_CARRY_SETS_SHARED 1
#define MG_CARRY_SETS_JOB_REGIONS 1
int mg_carry_sets_plan_host(const uint32_t* n_leaves /*[n_jobs]*/,
                            const uint32_t* n_rungs /*[n_jobs]*/,
                            const uint32_t* n_sets /*[n_jobs]*/, uint32_t n_jobs, uint32_t lanes,
                            uint32_t max_leaves, uint64_t* out_offsets, uint64_t* out_bytes,
                            uint64_t* out_leaf_stride_w);

/* The census of a pin ladder (csrc/mg_carry.h,
 * mg_carry_census.hip): mg_carry_ladder's columns, and instead of the lowest
 * true column alone a verdict census of every rung and `walkers` (W) start
 * columns per job — why a ladder missed, and where a walk would begin.
 * A job is a ladder job whose program carries its verdict mask as probes
 * mask_probe0 .. (mythril_amd/census.py mask_probes; load the census_view), and
 * its n_roots.  Columns are mg_carry_ladder's: C = R x lanes, R the batch's
 * largest n_rungs.  Rung r of job j is censused over its own columns
 * r x lanes .. r x lanes + lanes - 1 as mg_census does over candidates, with
 * column numbers for indices; the surplus columns of a job with fewer rungs
 * than R are evaluated and not counted.
 * counts: [n_jobs][R][5 x max_roots + 2] u64.  Block (j, r) holds, at its
 * front and for n = n_roots of job j, the counters as the device keeps them:
 * pass [n], first_block [n], sole_block [n], nfail_hist [n + 1], sole_index
 * [n] (all ones: none) and best = failing roots << 53 | column (all ones: no
 * column).  Blocks of rungs a job does not have, and words past a block's
 * 5 n + 2, are zero.
 * The start rule.  For rung r let (f_r, b_r) be its best: failing roots and
 * column.  The list of a job is first the bests of its rungs ordered by
 * (f_r, r) ascending; then, for r = 0 .. n_rungs - 1 and k = 0 .. n_roots - 1
 * in that order, every sole_index[r][k] that is set and is not b_r (1 failing
 * root each).  Start w is list[w]; past the end of the list it is list[0].
 * No column comes twice before the padding: rungs own disjoint column ranges;
 * a column is the sole candidate of at most one root; and a best with one
 * failing root is the lowest sole column of that root, the entry the rule
 * leaves out.  start_col [n_jobs][W], start_nfail [n_jobs][W], starts
 * [n_jobs][W][max_leaves][8]: the columns, their failing roots and their leaf
 * rows, zero past the program's leaves.  Start 0 is the ladder's answer: when
 * start_nfail[j][0] is 0, start_col[j][0] is mg_carry_ladder's first, its
 * rung start_col / lanes and starts[j][0] its leaves.
 * One call is a fixed sequence whatever n_jobs, with no host synchronisation
 * inside: one upload (descriptors, records, masks, rows, generator tables and
 * every counter block preset), the rung fill launch, one eval-mode interpreter
 * launch over the job axis at C candidates writing every job's probe region,
 * the census launch (grid tiles x R x jobs), the starts launch (one block per
 * job), one download.  mg_last_kernel_ms covers the four launches.  fill_out:
 * as mg_carry_ladder.
 * Refused with MG_E_ARG before any upload or launch, the message beginning
 * "carry_census:": whatever mg_carry_ladder refuses; walkers outside
 * 1..MG_CARRY_MAX_WALKERS; n_roots outside 1..1024 or above max_roots; mask
 * probes outside the program's probes. */
#define MG_CARRY_MAX_WALKERS 64u
typedef struct mg_carry_census_job {
    mg_carry_ladder_job ladder;
    uint32_t n_roots;           /* 1..1024 */
    uint32_t mask_probe0;       /* the first probe of the verdict mask */
} mg_carry_census_job;
int mg_carry_census(mg_ctx* ctx, const mg_carry_census_job* jobs, uint32_t n_jobs,
                    const mg_gen* gen, uint32_t lanes, uint32_t walkers, uint32_t max_roots,
                    uint32_t max_leaves, uint64_t* counts /*[n_jobs][R][5 max_roots + 2]*/,
                    int64_t* start_col /*[n_jobs][W]*/, uint32_t* start_nfail /*[n_jobs][W]*/,
                    uint32_t* starts /*[n_jobs][W][max_leaves][8]*/,
                    uint32_t* fill_out /*NULL, or every job's leaf region copied back*/);
/* Host-only (no GPU): the plan of the device buffer mg_carry_census uses.
 * out_offsets: mg_carry_ladder_plan_host's table — the same regions under the
 * same indices — followed by MG_CARRY_CENSUS_SHARED entries (the census
 * records) and MG_CARRY_CENSUS_JOB_REGIONS per job (its counter blocks, its
 * probe region).  In address order: descriptors, records, first words, every
 * job's masks, rows and generators — at the ladder's own offsets —, the census
 * records, every job's counter blocks (mg_census_words(n_roots) x n_rungs u64),
 * the output block, all leaf regions (the ladder's stride), all probe regions
 * (*out_probe_stride_w: the batch's largest n_probes x 8 x C words rounded up
 * to 256 bytes); every region 256-byte aligned.  MG_E_ARG for what
 * mg_carry_ladder_plan_host refuses, walkers outside 1..64, an n_roots outside
 * 1..1024, mask probes outside n_probes and sizes beyond 64 bits. */
#define MG_CARRY_CENSUS_SHARED 1
#define MG_CARRY_CENSUS_JOB_REGIONS 2
int mg_carry_census_plan_host(const uint32_t* n_leaves /*[n_jobs]*/,
                              const uint32_t* n_rungs /*[n_jobs]*/,
                              const uint32_t* n_roots /*[n_jobs]*/,
                              const uint32_t* n_probes /*[n_jobs]*/,
                              const uint32_t* mask_probe0 /*[n_jobs]*/, uint32_t n_jobs,
                              uint32_t lanes, uint32_t walkers, uint32_t max_leaves,
                              uint64_t* out_offsets, uint64_t* out_bytes,
                              uint64_t* out_leaf_stride_w, uint64_t* out_probe_stride_w);
/* Host-only (no GPU): the start rule on one job's counter blocks
 * ([n_rungs][5 n_roots + 2] u64, one after the other): start_col and
 * start_nfail [walkers]; -1 and 0xFFFFFFFF when no rung counted a column.
 * MG_E_ARG for a null pointer and counts out of range. */
int mg_carry_starts_host(const uint64_t* counts, uint32_t n_roots, uint32_t n_rungs,
                         uint32_t walkers, int64_t* start_col, uint32_t* start_nfail);

/* Corpus batches: many programs, one launch.  Device-pointer API for
 * resident benchmarking; stream is a hipStream_t (NULL = the context's own
 * stream, which the synchronous calls also use).
 *   d_root_bits : device [n_progs][ceil(n_assign/64)] u64 (may be NULL)
 *   d_first_sat : device [n_progs] u64, atomicMin'ed (preset to ~0)
 * Launches may be queued on several caller streams: freeing a program or a
 * batch waits for the last launch on every stream the context has seen
 * before its device block is reused.                                       */
int mg_batch_create(mg_ctx* ctx, const mg_prog* const* progs, uint32_t n_progs, mg_batch** out);
void mg_batch_free(mg_batch* batch);
int mg_batch_eval_gen(mg_ctx* ctx, mg_batch* batch, uint64_t seed, uint64_t first_index,
                      uint64_t n_assign, uint64_t* d_root_bits, uint64_t* d_first_sat,
                      void* stream);

/* Batched witness search (replaces the per-state Constraints.is_possible ->
 * get_model loop at mythril/laser/ethereum/svm.py:201-203 and :257-262):
 * for every program of the batch, the smallest candidate index in
 * [gen->first_index, gen->first_index + n_cand) that satisfies it, or -1, in
 * first_sat[n_progs].  All programs share each launch; waves of programs
 * already solved stop consuming lanes, with no host round trip.
 * witness_leaves (may be NULL): [n_progs][max_leaves][8] u32, the leaf values
 * of each solved program's witness (one regeneration launch for all);
 * max_leaves must be >= the batch's largest leaf count. */
int mg_batch_search(mg_ctx* ctx, mg_batch* batch, const mg_gen* gen, uint64_t n_cand,
                    int64_t* first_sat, uint32_t* witness_leaves, uint32_t max_leaves);
/* mg_batch_search plus, in the same regeneration launch, each solved
 * program's probe values at its witness (witness_probes: [n_progs]
 * [max_probes][8] u32, max_probes >= the batch's largest probe count;
 * witness_leaves must be given too): a solve-mode program's derived leaves
 * and argument-keyed table keys, so a batch of hits needs no per-hit
 * mg_eval_gen (round 5). */
int mg_batch_search_probes(mg_ctx* ctx, mg_batch* batch, const mg_gen* gen, uint64_t n_cand,
                           int64_t* first_sat, uint32_t* witness_leaves, uint32_t max_leaves,
                           uint32_t* witness_probes, uint32_t max_probes);
/* The regeneration launch of mg_batch_search_probes with caller-given
 * indices: pair i is candidate indices[i] of progs[i] under `seed`, its leaf
 * values in leaves[i][max_leaves][8] and, when probes is not NULL, its probe
 * values in probes[i][max_probes][8] — what mg_eval_gen returns for one lane
 * at that index.  One launch for all pairs (65535 per launch).  A program may
 * appear in many pairs.  Index -1 leaves the pair's rows zero.  It serves the
 * misses of Constraints.is_possible, as mg_census does: the starts of a
 * group's repair walks and the best candidate of its miss report are
 * candidates its census names.  MG_E_ARG before any launch, the message
 * beginning "batch_witness:": a null pointer, a program of another context,
 * an index below -1, rows narrower than a program's leaves or probes. */
int mg_batch_witness(mg_ctx* ctx, const mg_prog* const* progs, const int64_t* indices, uint32_t n,
                     uint64_t seed, uint32_t* leaves, uint32_t max_leaves, uint32_t* probes,
                     uint32_t max_probes);

/* Compiled programs (batch path without interpretive dispatch; built on the
 * host by mythril_amd/jit.py): ``image`` is a gfx950 code object holding the
 * straight-line code of programs[0..n_progs) and their entry table
 * ``mg_jit_table``: row 0 = (MG_JIT_MAGIC, the first 16 hex digits of
 * mg_asm_digest() of the interpreter the code was generated for — pinned
 * registers, descriptor layout), row i + 1 = (entry offset of program i from
 * the table, fingerprint of the records program i was compiled from: every
 * word of its records with handler ids in word 0).  Attaching points each
 * program's descriptor at its code; evaluations of those programs — and
 * batches created afterwards — then run the code instead of dispatching
 * records (same results, same kernel).  MG_E_ARG when the header names
 * another interpreter, an entry lies outside the image's executable sections
 * or a row's fingerprint is not the loaded program's (code compiled for other
 * records — another opcode, variant, operand or constant — is never entered).
 * Same role as mg_load_program for Optimize.add (solver.py:28-37),
 * specialised for the batched evaluation (laser/smt/model.py:44-59). */
#define MG_JIT_MAGIC 0x4D474A4954763033ull   /* "MGJITv03" */
int mg_jit_attach(mg_ctx* ctx, mg_prog* const* progs, uint32_t n_progs, const void* image,
                  size_t image_size, mg_jit** out);
/* Back to the interpreter for those programs; unloads the code object.
 * Free batches created while attached first. */
void mg_jit_detach(mg_jit* jit);

/* Keccak-256 (0x01 padding) of n messages, one GPU lane per message.
 *   data/offsets/lens describe the messages in one host byte buffer;
 *   out: n x 32 bytes. */
int mg_keccak256(mg_ctx* ctx, const uint8_t* data, const uint64_t* offsets,
                 const uint32_t* lens, uint32_t n, uint8_t* out);

/* The HIP runtime this library runs on in this process: hipRuntimeGetVersion
 * and the file of the libamdhip64 it resolved to (a process that loaded
 * PyTorch first binds torch's bundled runtime; bench.py reports both). */
int mg_runtime_info(int* hip_version, char* path, size_t path_len);
/* Library/ABI version (no GPU needed). */
int mg_version(void);
/* Digest of the generated gfx950 assembly the library was built from (no
 * GPU needed; mythril_amd/asmgen.py digest()): of the 16-slot interpreter,
 * and of the interpreter of any layout (NULL for a slot count it lacks). */
const char* mg_asm_digest(void);
const char* mg_asm_digest_layout(uint32_t nreg);
/* Host-only (no GPU): translate a validated IR program compiled for the
 * nreg-slot layout into the 8-word records of that layout's assembly
 * interpreter, given its handler offset table (mg_load_program does this
 * with the table queried from the device).
 *   records: up to (2 * n_ins + 3) x 8 words (a WAITVM record may precede
 *   an instruction); masks: mask entries appended after the
 *   program's n_consts constants (8 words each).  Sizes are returned in
 *   *n_record_words / *n_mask_words; MG_E_ARG when a buffer is too small. */
int mg_translate(const uint32_t* code, uint32_t n_ins, uint32_t n_consts, uint32_t n_lds,
                 uint32_t nreg, const uint32_t* handler_off, uint32_t n_handlers,
                 uint32_t* records, uint32_t max_record_words, uint32_t* n_record_words,
                 uint32_t* masks, uint32_t max_mask_words, uint32_t* n_mask_words);
/* Build configuration (no GPU needed): out[0..3] = version, MG_NREG (the
 * most slots any layout has; mg_layouts lists them), MG_MAX_LDS,
 * MG_MAX_PSLOTS. */
int mg_config(uint32_t* out, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif

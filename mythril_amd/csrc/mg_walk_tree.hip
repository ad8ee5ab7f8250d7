// mg_walk_tree — the scored walk with tree distances (DESIGN.md §3.11;
// specification: mythril_amd/repair.py walk_ref with tree_score_ref).
//
// A round is the round of mg_walk.hip with one kernel exchanged:
//   mg_walk_mutate      (mg_walk.hip, unchanged)
//   the interpreter     writes every neighbour's root mask, atom mask and
//                       residual probes
//   mg_walk_tree_score  lane j scores neighbour j (mg_walk_tree.h): a failing
//                       tree root costs the value of its postfix program over
//                       the atoms; walker w's key is min over its lanes of
//                       nfail << 40 | cost << 20 | lane, reduced as
//                       mg_walk_score reduces it
//   mg_walk_adopt       (mg_walk.hip, unchanged)
// The stack of the postfix programs lives in LDS, [8][256] u32 per block:
// its pointer is wave-uniform but dynamic, and a per-lane array indexed by it
// would go to scratch.  Lane t only touches column t, so no barrier is needed.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_walk_round.h"    // the score body, shared with mg_walk_batch_score

hipError_t mg_launch_walk_adopt(uint32_t* d_bases, const mg_leafgen* d_gen,
                                const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                                uint32_t r, uint32_t lanes, uint32_t walkers, uint32_t max_rounds,
                                mg_walk_state* d_state, uint32_t* d_trace, hipStream_t stream);

__global__ __launch_bounds__(MG_WALK_BLOCK) void mg_walk_tree_score(
    const uint32_t* __restrict__ masks, const uint32_t* __restrict__ amasks,
    const uint32_t* __restrict__ resid, const uint32_t* __restrict__ roots,
    const uint32_t* __restrict__ atoms, const uint32_t* __restrict__ code, uint32_t lanes,
    uint32_t n_roots, mg_walk_state* __restrict__ st) {
    mg_walk_score_body(masks, amasks, resid, roots, atoms, code, lanes, n_roots, st);
}

// score with the tree tables, then the adopt of mg_walk.hip.  The tables must
// have passed mg_walk_tree_ok (mg_walk_tree checks them before it uploads).
hipError_t mg_launch_walk_tree_pick(const uint32_t* d_masks, const uint32_t* d_amasks,
                                    const uint32_t* d_resid, const uint32_t* d_roots,
                                    const uint32_t* d_atoms, const uint32_t* d_code,
                                    uint32_t lanes, uint32_t walkers, uint32_t n_roots,
                                    uint32_t* d_bases, const mg_leafgen* d_gen,
                                    const uint32_t* d_consts, uint32_t n_leaves, uint64_t seed,
                                    uint32_t r, uint32_t max_rounds, mg_walk_state* d_state,
                                    uint32_t* d_trace, hipStream_t stream) {
    if (walkers < 1 || walkers > MG_WALK_MAX_WALKERS || lanes < 1 || lanes > MG_REPAIR_MAX_LANES ||
        n_leaves == 0 || n_roots == 0 || n_roots > MG_WT_MAX_ROOTS || r >= max_rounds ||
        r >= MG_REPAIR_MAX_ROUNDS)
        return hipErrorInvalidValue;
    const uint32_t blocks = mg_walk_grid_blocks(lanes);
    hipLaunchKernelGGL(mg_walk_tree_score, dim3(blocks, walkers), dim3(MG_WALK_BLOCK), 0, stream, d_masks,
                       d_amasks, d_resid, d_roots, d_atoms, d_code, lanes, n_roots, d_state);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return mg_launch_walk_adopt(d_bases, d_gen, d_consts, n_leaves, seed, r, lanes, walkers,
                                max_rounds, d_state, d_trace, stream);
}

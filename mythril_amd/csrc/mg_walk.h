/* The scoring function of the scored walk (mg_walk), for
 * host and device: the key (failing roots, cost) of one neighbour from its
 * verdict mask, its residual probes and the residual table, so the kernel
 * that scores the neighbours (mg_walk_score) and the host entry the CPU suite
 * compares with the specification (mg_walk_score_host) run the same code.
 * Specification, bit for bit: mythril_amd/repair.py score_ref.
 *
 * table[k] = kind << 16 | probe index among the residual probes.  A root k
 * that fails (its mask bit is clear) costs its distance d_k:
 *   MG_WALK_FLAT       1
 *   MG_WALK_HAMMING    max(1, popcount(R))    R = a xor b of a root a = b
 *   MG_WALK_MAGNITUDE  1 + bitlen(R)          R = a - b of an order root
 * cost = the sum of d_k over the failing roots, so cost >= nfail, and at most
 * 1024 * 257 < 2^19.  Whether a root holds is read from the mask alone.
 *
 * Walker w of mg_walk runs the move function of mg_repair.h under the seed
 * seed ^ w * MG_WALK_CW. */
#ifndef MG_WALK_H
#define MG_WALK_H

#include <stdint.h>
#include "mg_repair.h"

#define MG_WALK_CW 0x8CB92BA72F3D8DD7ull
#define MG_WALK_FLAT 0u
#define MG_WALK_HAMMING 1u
#define MG_WALK_MAGNITUDE 2u
#define MG_WALK_KINDS 3u
#define MG_WALK_MAX_WALKERS 64u
/* key = nfail << 40 | cost << 20 | lane */
#define MG_WALK_NFAIL_SHIFT 40
#define MG_WALK_COST_SHIFT 20
#define MG_WALK_FIELD 0xFFFFFu

#define MG_WALK_FN MG_REPAIR_FN

/* device state of one walker (mg_walk.hip): the round's key (minimum over
 * the walker's lanes, ~0 between rounds), then the 8 bytes the host reads
 * back: the base's failing roots and cost (~0 before round 0) */
struct mg_walk_state {
    unsigned long long key;
    uint32_t nfail;
    uint32_t cost;
};

MG_WALK_FN uint64_t mg_walk_seed(uint64_t seed, uint32_t w) {
    return seed ^ ((uint64_t)w * MG_WALK_CW);
}

/* OR over the lanes that share one pass through the scoring loop: the wave
 * on the device (every lane of it calls this, converged), one lane on the
 * host */
MG_WALK_FN uint32_t mg_walk_any(uint32_t x) {
#ifdef __HIP_DEVICE_COMPILE__
    for (int off = 32; off > 0; off >>= 1) x |= __shfl_xor(x, off, 64);
    return __builtin_amdgcn_readfirstlane(x);
#else
    return x;
#endif
}

MG_WALK_FN uint32_t mg_walk_popc(uint32_t x) {
#ifdef __HIP_DEVICE_COMPILE__
    return __popc(x);
#else
    return (uint32_t)__builtin_popcount(x);
#endif
}

MG_WALK_FN uint32_t mg_walk_clz(uint32_t x) {    /* x != 0 */
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__clz((int)x);
#else
    return (uint32_t)__builtin_clz(x);
#endif
}

/* (nfail, cost) of lane `col`.  masks: the rows of the verdict mask, word q
 * of the lane at masks[q * stride + col]; resid: the residual probes, limb i
 * of probe p at resid[(p * 8 + i) * stride + col].  A lane that is not
 * `active` reads nothing and returns (0, 0); it still takes part in
 * mg_walk_any.  The eight limb rows of a residual are read only when some
 * lane of the wave fails its root (a wave-uniform branch), and then by the
 * failing lanes alone. */
MG_WALK_FN void mg_walk_score_lane(const uint32_t* masks, const uint32_t* resid, uint64_t stride,
                                   uint64_t col, const uint32_t* table, uint32_t n_roots,
                                   bool active, uint32_t* out_nfail, uint32_t* out_cost) {
    const uint32_t n_words = (n_roots + 31) / 32;
    uint32_t nfail = 0, cost = 0;
    for (uint32_t q = 0; q < n_words; ++q) {
        const uint32_t bits = n_roots - 32 * q < 32 ? n_roots - 32 * q : 32;
        const uint32_t valid = bits == 32 ? ~0u : (1u << bits) - 1u;   /* bits >= n_roots: ignored */
        const uint32_t fails = active ? ~masks[(uint64_t)q * stride + col] & valid : 0u;
        nfail += mg_walk_popc(fails);
        uint32_t any = mg_walk_any(fails);
        while (any) {                                                  /* wave-uniform */
            const uint32_t b = 31u - mg_walk_clz(any & (0u - any));
            any &= any - 1u;
            const uint32_t entry = table[32 * q + b];                  /* wave-uniform load */
            const uint32_t kind = entry >> 16, p = entry & 0xFFFFu;
            const bool f = (fails >> b & 1u) != 0;
            if (kind == MG_WALK_FLAT) {
                cost += f ? 1u : 0u;
            } else if (f) {
                uint32_t pop = 0, len = 0;
                for (uint32_t i = 0; i < 8; ++i) {
                    const uint32_t limb = resid[((uint64_t)p * 8 + i) * stride + col];
                    pop += mg_walk_popc(limb);
                    if (limb) len = 32 * i + 32 - mg_walk_clz(limb);
                }
                cost += kind == MG_WALK_HAMMING ? (pop ? pop : 1u) : 1u + len;
            }
        }
    }
    *out_nfail = nfail;
    *out_cost = cost;
}

MG_WALK_FN unsigned long long mg_walk_key(uint32_t nfail, uint32_t cost, uint32_t lane) {
    return ((unsigned long long)nfail << MG_WALK_NFAIL_SHIFT) |
           ((unsigned long long)cost << MG_WALK_COST_SHIFT) | lane;
}

#endif

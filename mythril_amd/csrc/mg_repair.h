/* The move function of the local search (mg_repair), for
 * host and device: the neighbour that lane j of round r evaluates, as a
 * function of (base assignment, seed, r, j, lanes) alone, so the kernel that
 * writes the neighbours (mg_repair_mutate), the kernel that adopts the best
 * one (mg_repair_adopt: no gather) and the host entry the CPU suite compares
 * with the specification (mg_repair_mutate_host) run the same code.
 * Specification, bit for bit: mythril_amd/repair.py mutate_ref.
 *
 * Lane 0 is the base unchanged.  Lanes 1 .. lanes / 2 - 1 apply one move, the
 * others two, the second to the result of the first.  Move m (0, 1) of lane
 * j of round r draws two 64-bit words, d = 0, 1:
 *   s  = seed ^ r * MG_REPAIR_CR ^ j * MG_REPAIR_CJ ^ (2 m + d + 1) * MG_REPAIR_CD
 *   s += 0x9E3779B97F4A7C15; u = s ^ (s >> 32); z = u * 0xBF58476D1CE4E5B9
 *   h_d = z ^ (z >> 32)                 (the generator's v9 mix, mythgpu.h)
 * and, with w the leaf's width and mulhi(a, n) = (a * n) >> 32:
 *   leaf = mulhi(lo(h_0), n_leaves)     kind = mulhi(hi(h_0), 6)
 *   a = lo(h_1), c = hi(h_1), b = mulhi(a, w)
 *   kind 0  flip bit b
 *   kind 1  add (c even) or subtract (c odd) 2^b modulo 2^w
 *   kind 2  byte mulhi(a, ceil(w / 8)) becomes c & 0xFF
 *   kind 3  limb mulhi(a, ceil(w / 32)) becomes c
 *   kind 4  pool_n > 0: consts[pool_off + mulhi(a, pool_n)] + mulhi(c, 3) - 1
 *           (mod 2^256); else {0, 1, 2^(w-1), 2^w - 1}[c & 3]
 *   kind 5  the value of leaf mulhi(a, n_leaves)
 * every result masked to w bits. */
#ifndef MG_REPAIR_H
#define MG_REPAIR_H

#include <stdint.h>
#include "mythgpu.h"

#define MG_REPAIR_CR 0xD6E8FEB86659FD93ull
#define MG_REPAIR_CJ 0xA0761D6478BD642Full
#define MG_REPAIR_CD 0xE7037ED1A0B428DBull
#define MG_REPAIR_KINDS 6u
#define MG_REPAIR_MAX_LANES (1u << 20)
#define MG_REPAIR_MAX_ROUNDS (1u << 16)

#define MG_REPAIR_FN static inline __attribute__((always_inline))
#ifdef __HIPCC__
#undef MG_REPAIR_FN
#define MG_REPAIR_FN __host__ __device__ static inline __attribute__((always_inline))
#endif

/* the moves of one lane: leaf[m] takes val[m], in order (n = 0, 1 or 2) */
struct mg_repair_moves {
    uint32_t n;
    uint32_t leaf[2];
    uint32_t kind[2];
    uint32_t val[2][8];
};

/* device state of one search (mg_repair.hip): the round's key (minimum of
 * nfail << 32 | lane, ~0 between rounds), then the 8 bytes the host reads
 * back: the base's failing roots (~0 before round 0) and the rounds done */
struct mg_repair_state {
    unsigned long long key;
    uint32_t base_nfail;
    uint32_t rounds;
};

MG_REPAIR_FN uint64_t mg_repair_hash(uint64_t seed, uint32_t r, uint32_t j, uint32_t draw) {
    uint64_t s = seed ^ ((uint64_t)r * MG_REPAIR_CR) ^ ((uint64_t)j * MG_REPAIR_CJ) ^
                 ((uint64_t)(draw + 1) * MG_REPAIR_CD);
    s += 0x9E3779B97F4A7C15ull;
    const uint64_t u = s ^ (s >> 32);
    const uint64_t z = u * 0xBF58476D1CE4E5B9ull;
    return z ^ (z >> 32);
}

MG_REPAIR_FN uint32_t mg_repair_mulhi(uint32_t a, uint32_t n) {
    return (uint32_t)(((uint64_t)a * n) >> 32);
}

MG_REPAIR_FN uint32_t mg_repair_moves_of(uint32_t j, uint32_t lanes) {
    return j == 0 ? 0u : (j < lanes / 2 ? 1u : 2u);
}

/* leaf `leaf` of the lane after its first `upto` moves */
MG_REPAIR_FN void mg_repair_leaf(const uint32_t* base, const mg_repair_moves& mv, uint32_t upto,
                                 uint32_t leaf, uint32_t* out) {
    const bool m0 = upto > 0 && mv.leaf[0] == leaf, m1 = upto > 1 && mv.leaf[1] == leaf;
    for (uint32_t k = 0; k < 8; ++k)
        out[k] = m1 ? mv.val[1][k] : (m0 ? mv.val[0][k] : base[(uint64_t)leaf * 8 + k]);
}

/* v += sign * 2^b (256 bits; limbs selected by comparison, no indexed access) */
MG_REPAIR_FN void mg_repair_addpow(uint32_t* v, uint32_t b, bool sub) {
    uint32_t carry = 0;
    for (uint32_t k = 0; k < 8; ++k) {
        const uint32_t t = (k == b >> 5) ? 1u << (b & 31) : 0u;
        if (!sub) {
            const uint64_t x = (uint64_t)v[k] + t + carry;
            v[k] = (uint32_t)x;
            carry = (uint32_t)(x >> 32);
        } else {
            const uint64_t x = (uint64_t)v[k] - t - carry;
            v[k] = (uint32_t)x;
            carry = (uint32_t)(x >> 32) & 1u;
        }
    }
}

MG_REPAIR_FN void mg_repair_mask(uint32_t* v, uint32_t w) {
    for (uint32_t k = 0; k < 8; ++k) {
        if (32 * k >= w) v[k] = 0;
        else if (w - 32 * k < 32) v[k] &= (1u << (w - 32 * k)) - 1u;
    }
}

/* The moves of lane j of round r over `base` ([n_leaves][8]); gen: the
 * program's leaf table (width, pool_off, pool_n are read), consts: its
 * constant table ([n_consts][8]). */
MG_REPAIR_FN void mg_repair_lane(const uint32_t* base, const mg_leafgen* gen,
                                 const uint32_t* consts, uint32_t n_leaves, uint64_t seed,
                                 uint32_t r, uint32_t j, uint32_t lanes, mg_repair_moves* mv) {
    mv->n = mg_repair_moves_of(j, lanes);
    for (uint32_t m = 0; m < 2; ++m) {
        mv->leaf[m] = 0;
        mv->kind[m] = 0;
        for (uint32_t k = 0; k < 8; ++k) mv->val[m][k] = 0;
    }
    for (uint32_t m = 0; m < mv->n; ++m) {
        const uint64_t h0 = mg_repair_hash(seed, r, j, 2 * m);
        const uint64_t h1 = mg_repair_hash(seed, r, j, 2 * m + 1);
        const uint32_t leaf = mg_repair_mulhi((uint32_t)h0, n_leaves);
        const uint32_t kind = mg_repair_mulhi((uint32_t)(h0 >> 32), MG_REPAIR_KINDS);
        const uint32_t a = (uint32_t)h1, c = (uint32_t)(h1 >> 32);
        const uint32_t w = gen[leaf].width;
        const uint32_t b = mg_repair_mulhi(a, w);
        uint32_t v[8];
        mg_repair_leaf(base, *mv, m, leaf, v);
        if (kind == 0) {
            for (uint32_t k = 0; k < 8; ++k)
                if (k == b >> 5) v[k] ^= 1u << (b & 31);
        } else if (kind == 1) {
            mg_repair_addpow(v, b, (c & 1u) != 0);
        } else if (kind == 2) {
            const uint32_t at = mg_repair_mulhi(a, (w + 7) / 8);
            const uint32_t sh = 8 * (at & 3);
            for (uint32_t k = 0; k < 8; ++k)
                if (k == at >> 2) v[k] = (v[k] & ~(0xFFu << sh)) | ((c & 0xFFu) << sh);
        } else if (kind == 3) {
            const uint32_t at = mg_repair_mulhi(a, (w + 31) / 32);
            for (uint32_t k = 0; k < 8; ++k)
                if (k == at) v[k] = c;
        } else if (kind == 4) {
            if (gen[leaf].pool_n > 0) {
                const uint32_t e = gen[leaf].pool_off + mg_repair_mulhi(a, gen[leaf].pool_n);
                const uint32_t delta = mg_repair_mulhi(c, 3);
                for (uint32_t k = 0; k < 8; ++k) v[k] = consts[(uint64_t)e * 8 + k];
                if (delta != 1) mg_repair_addpow(v, 0, delta == 0);
            } else {
                const uint32_t pick = c & 3u;
                for (uint32_t k = 0; k < 8; ++k)
                    v[k] = pick == 3 ? 0xFFFFFFFFu : (pick == 1 && k == 0 ? 1u : 0u);
                if (pick == 2) mg_repair_addpow(v, w - 1, false);
            }
        } else {
            mg_repair_leaf(base, *mv, m, mg_repair_mulhi(a, n_leaves), v);
        }
        mg_repair_mask(v, w);
        mv->leaf[m] = leaf;
        mv->kind[m] = kind;
        for (uint32_t k = 0; k < 8; ++k) mv->val[m][k] = v[k];
    }
}

#endif

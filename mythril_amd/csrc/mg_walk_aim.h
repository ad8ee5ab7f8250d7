/* The aimed moves of mg_walk_aim, for host and device: the
 * neighbour that lane j of round r evaluates, as a function of (base, the
 * base's residual values, seed, r, j, lanes, aim table) alone, so the kernel
 * that writes the neighbours (mg_walk_aim_mutate), the kernel that adopts the
 * best one (mg_walk_aim_adopt: no gather of leaves) and the host entry the
 * CPU suite compares with the specification (mg_walk_aim_mutate_host) run the
 * same code.  Specification, bit for bit: mythril_amd/repair.py
 * aim_mutate_ref.
 *
 * A positive equality a = b carries the residual probe R = a xor b.  Where
 * side a is made of leaves, a xor R = b: flipping in a's leaves the bits set
 * in R makes the equality hold in one move.  The aim table lists such sides:
 *   entries[3 e ..]  residual probe, first piece, pieces (1 .. 64)
 *   pieces[4 p ..]   leaf, leaf_bit, value_bit, len
 * and piece p of entry e does
 *   leaf ^= ((R >> value_bit) & (2^len - 1)) << leaf_bit
 * with R the entry's residual under the walker's base.
 *
 * L = the entries whose R is non-zero under the base, in table order (empty
 * in round 0, where no residual is known), cap = lanes / 8, n1 = min(|L|,
 * cap).  Lane 0 is the base; lanes 1 .. n1 are the base with entry
 * L[(j - 1 + r n1) mod |L|] applied and nothing else; lanes n1 + 1 .. 2 n1
 * take the same entry for j - n1, and then the moves mg_repair_lane gives
 * lane j (computed from the base) are written over the result: a plain move
 * wins a leaf it shares with a piece.  Every other lane is mg_repair_lane's
 * neighbour. */
#ifndef MG_WALK_AIM_H
#define MG_WALK_AIM_H

#include <stdint.h>
#include "mg_repair.h"

#define MG_AIM_MAX_ENTRIES 256u
#define MG_AIM_MAX_PIECES 64u
#define MG_AIM_NONE 0xFFFFFFFFu
/* words of one walker's live list: |L|, then L */
#define MG_AIM_LIVE_WORDS (1u + MG_AIM_MAX_ENTRIES)

#define MG_AIM_FN MG_REPAIR_FN

/* Everything the kernels index by: residual index < n_resid, 1 .. 64 pieces
 * per entry inside the piece array, leaf < n_leaves, leaf_bit + len <= the
 * leaf's width, value_bit + len <= 256, at most 256 entries.  An empty table
 * (no entry, no piece) is valid. */
static inline bool mg_walk_aim_ok(const uint32_t* entries, uint32_t n_entries,
                                  const uint32_t* pieces, uint32_t n_pieces,
                                  const mg_leafgen* gen, uint32_t n_leaves, uint32_t n_resid) {
    if (n_entries > MG_AIM_MAX_ENTRIES) return false;
    if ((n_entries && !entries) || (n_pieces && !pieces)) return false;
    if (n_entries && !gen) return false;
    for (uint32_t e = 0; e < n_entries; ++e) {
        const uint32_t p = entries[3 * (size_t)e], off = entries[3 * (size_t)e + 1],
                       cnt = entries[3 * (size_t)e + 2];
        if (p >= n_resid) return false;
        if (cnt < 1 || cnt > MG_AIM_MAX_PIECES) return false;
        if (off > n_pieces || cnt > n_pieces - off) return false;
        for (uint32_t q = off; q < off + cnt; ++q) {
            const uint32_t leaf = pieces[4 * (size_t)q], leaf_bit = pieces[4 * (size_t)q + 1],
                           value_bit = pieces[4 * (size_t)q + 2], len = pieces[4 * (size_t)q + 3];
            if (leaf >= n_leaves) return false;
            const uint32_t w = gen[leaf].width;
            if (w > 256 || len < 1 || len > 256) return false;
            if (leaf_bit > w || len > w - leaf_bit) return false;
            if (value_bit > 256 || len > 256 - value_bit) return false;
        }
    }
    return true;
}

/* is entry e live: its residual, limb i at rvals[(p * 8 + i) * stride], is
 * not zero */
MG_AIM_FN bool mg_walk_aim_is_live(const uint32_t* entries, uint32_t e, const uint32_t* rvals,
                                   uint64_t stride) {
    const uint32_t p = entries[3 * (uint64_t)e];
    uint32_t any = 0;
    for (uint32_t i = 0; i < 8; ++i) any |= rvals[((uint64_t)p * 8 + i) * stride];
    return any != 0;
}

/* The position in L of the entry that lane j of round r applies, or
 * MG_AIM_NONE; *plain: do mg_repair_lane's moves of lane j apply as well. */
MG_AIM_FN uint32_t mg_walk_aim_pick(uint32_t n_live, uint32_t r, uint32_t j, uint32_t lanes,
                                    bool* plain) {
    const uint32_t cap = lanes / 8;
    const uint32_t n1 = n_live < cap ? n_live : cap;
    *plain = j > n1;
    if (j == 0 || j > 2 * n1) return MG_AIM_NONE;
    const uint32_t jj = j > n1 ? j - n1 : j;
    return (uint32_t)(((uint64_t)(jj - 1) + (uint64_t)r * n1) % n_live);
}

/* v >>= s, 0 <= s < 256: whole limbs by halving steps over fixed indices,
 * then a funnel over neighbouring limbs (no limb is indexed by s) */
MG_AIM_FN void mg_walk_aim_shr(uint32_t* v, uint32_t s) {
    if (s & 128u)
        for (uint32_t k = 0; k < 8; ++k) v[k] = k + 4 < 8 ? v[k + 4] : 0u;
    if (s & 64u)
        for (uint32_t k = 0; k < 8; ++k) v[k] = k + 2 < 8 ? v[k + 2] : 0u;
    if (s & 32u)
        for (uint32_t k = 0; k < 8; ++k) v[k] = k + 1 < 8 ? v[k + 1] : 0u;
    const uint32_t b = s & 31u;
    for (uint32_t k = 0; k < 8; ++k) {
        const uint64_t pair = ((uint64_t)(k + 1 < 8 ? v[k + 1] : 0u) << 32) | v[k];
        v[k] = (uint32_t)(pair >> b);
    }
}

/* v <<= s, 0 <= s < 256 */
MG_AIM_FN void mg_walk_aim_shl(uint32_t* v, uint32_t s) {
    if (s & 128u)
        for (uint32_t k = 8; k-- > 0;) v[k] = k >= 4 ? v[k - 4] : 0u;
    if (s & 64u)
        for (uint32_t k = 8; k-- > 0;) v[k] = k >= 2 ? v[k - 2] : 0u;
    if (s & 32u)
        for (uint32_t k = 8; k-- > 0;) v[k] = k >= 1 ? v[k - 1] : 0u;
    const uint32_t b = s & 31u;
    for (uint32_t k = 8; k-- > 0;) {
        const uint64_t pair = ((uint64_t)v[k] << 32) | (k >= 1 ? v[k - 1] : 0u);
        v[k] = (uint32_t)((pair << b) >> 32);
    }
}

/* what one piece xors into its leaf: ((R >> value_bit) & mask(len)) <<
 * leaf_bit.  v: R on entry, the result on return. */
MG_AIM_FN void mg_walk_aim_piece(uint32_t* v, uint32_t leaf_bit, uint32_t value_bit,
                                 uint32_t len) {
    mg_walk_aim_shr(v, value_bit);
    mg_repair_mask(v, len);
    mg_walk_aim_shl(v, leaf_bit);
}

/* Host only: L of a base with residual values rvals ([n_resid][8]; NULL:
 * round 0, no residual known) into live[1 ..], |L| into live[0]. */
static inline void mg_walk_aim_live(const uint32_t* entries, uint32_t n_entries,
                                    const uint32_t* rvals, uint32_t* live) {
    uint32_t n = 0;
    for (uint32_t e = 0; rvals && e < n_entries; ++e)
        if (mg_walk_aim_is_live(entries, e, rvals, 1)) live[1 + n++] = e;
    live[0] = n;
}

/* Lane j of round r applied to `dst` ([n_leaves][8] at dst[(leaf * 8 + k) *
 * stride], holding the base's values): the pieces of its entry xored in,
 * then its plain moves written over.  rvals: the base's residual values
 * ([n_resid][8]), live: its L.  *report (or NULL): mg_repair_lane's moves of
 * the lane, n = 0 where they do not apply; returns the entry applied or
 * MG_AIM_NONE. */
MG_AIM_FN uint32_t mg_walk_aim_lane(const uint32_t* base, const mg_leafgen* gen,
                                    const uint32_t* consts, uint32_t n_leaves, uint64_t seed,
                                    uint32_t r, uint32_t j, uint32_t lanes,
                                    const uint32_t* entries, const uint32_t* pieces,
                                    const uint32_t* rvals, const uint32_t* live, uint32_t* dst,
                                    uint64_t stride, mg_repair_moves* report) {
    bool plain;
    const uint32_t at = mg_walk_aim_pick(live[0], r, j, lanes, &plain);
    mg_repair_moves mv;
    mg_repair_lane(base, gen, consts, n_leaves, seed, r, j, lanes, &mv);
    if (!plain) mv.n = 0;
    if (report) *report = mv;
    const bool m0 = mv.n > 0, m1 = mv.n > 1;
    const uint32_t leaf0 = mv.leaf[0], leaf1 = mv.leaf[1];
    uint32_t e = MG_AIM_NONE;
    if (at != MG_AIM_NONE) {
        e = live[1 + at];
        const uint32_t p = entries[3 * (uint64_t)e], off = entries[3 * (uint64_t)e + 1],
                       cnt = entries[3 * (uint64_t)e + 2];
        for (uint32_t q = off; q < off + cnt; ++q) {
            const uint32_t leaf = pieces[4 * (uint64_t)q];
            if ((m0 && leaf0 == leaf) || (m1 && leaf1 == leaf)) continue;
            uint32_t v[8];
            for (uint32_t k = 0; k < 8; ++k) v[k] = rvals[(uint64_t)p * 8 + k];
            mg_walk_aim_piece(v, pieces[4 * (uint64_t)q + 1], pieces[4 * (uint64_t)q + 2],
                              pieces[4 * (uint64_t)q + 3]);
            for (uint32_t k = 0; k < 8; ++k)
                if (v[k]) dst[((uint64_t)leaf * 8 + k) * stride] ^= v[k];
        }
    }
    if (m0)
        for (uint32_t k = 0; k < 8; ++k) dst[((uint64_t)leaf0 * 8 + k) * stride] = mv.val[0][k];
    if (m1)
        for (uint32_t k = 0; k < 8; ++k) dst[((uint64_t)leaf1 * 8 + k) * stride] = mv.val[1][k];
    return e;
}

#endif

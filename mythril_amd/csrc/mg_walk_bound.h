/* The aimed moves of mg_walk_bound, for host and device:
 * the lane function of mg_walk_aim.h with a wider aim table, whose entries
 * are the XOR entries of §3.12 or order entries.  The kernel that writes the
 * neighbours (mg_walk_bound_mutate), the kernel that adopts the best one
 * (mg_walk_bound_adopt) and the host entry the CPU suite compares with the
 * specification (mg_walk_bound_mutate_host) run the same code.
 * Specification, bit for bit: mythril_amd/repair.py bound_mutate_ref.
 *
 * An order atom lo < hi / lo <= hi carries the residual probe D = lo - hi.
 * Where side lo is made of leaves, lo - D - s = hi - s (s = 1 for the strict
 * orders) makes the order hold in one move; where hi is, hi + D + s = lo + s.
 *   entries[5 e ..]  residual probe, first piece, pieces (1 .. 64), mode, truth
 *   pieces[4 p ..]   leaf, leaf_bit, value_bit, len
 *   fixed[8 e ..]    the side's numeral bits (a numeral operand of a concat)
 *   mode             0 XOR, 1 LOW, 2 LOW_STRICT, 3 HIGH, 4 HIGH_STRICT
 *   truth            1 << 31 | i: bit i of the atom mask; else bit k of the
 *                    root mask (XOR entries: 0, and fixed is 0)
 * An order entry gathers the side's value from the base,
 *   V = fixed | OR over pieces ((base[leaf] >> leaf_bit) & mask(len)) << value_bit
 * takes T = V - D - s (LOW) or V + D + s (HIGH) mod 2^256, and scatters it in
 * piece order into the lane's current value of each leaf:
 *   leaf = leaf & ~(mask(len) << leaf_bit) | ((T >> value_bit) & mask(len)) << leaf_bit
 * Bits at or above the side's width are never scattered and carries only go
 * upward, so no width is needed.
 *
 * L = the live entries in table order (empty in round 0): an XOR entry is
 * live iff its residual is not 0 under the base, an order entry iff its truth
 * bit is clear on the base.  The mask state of a base is its root-mask rows,
 * then its atom-mask rows: mask bit k is bit k % 32 of word k / 32.  The lane
 * layout is mg_walk_aim's exactly (mg_walk_aim_pick). */
#ifndef MG_WALK_BOUND_H
#define MG_WALK_BOUND_H

#include <stdint.h>
#include "mg_walk_aim.h"

#define MG_BOUND_XOR 0u
#define MG_BOUND_LOW 1u
#define MG_BOUND_LOW_STRICT 2u
#define MG_BOUND_HIGH 3u
#define MG_BOUND_HIGH_STRICT 4u
#define MG_BOUND_ATOM 0x80000000u
/* words of the root (atom) mask rows of one lane */
#define MG_BOUND_MASK_WORDS(n) ((((n) + 255u) / 256u) * 8u)

/* Everything mg_walk_aim_ok checks, and: mode <= 4, the truth index below
 * n_atoms, respectively n_roots, truth and fixed zero for XOR entries. */
static inline bool mg_walk_bound_ok(const uint32_t* entries, uint32_t n_entries,
                                    const uint32_t* pieces, uint32_t n_pieces,
                                    const uint32_t* fixed, const mg_leafgen* gen,
                                    uint32_t n_leaves, uint32_t n_resid, uint32_t n_roots,
                                    uint32_t n_atoms) {
    if (n_entries > MG_AIM_MAX_ENTRIES) return false;
    if ((n_entries && (!entries || !fixed)) || (n_pieces && !pieces)) return false;
    if (n_entries && !gen) return false;
    for (uint32_t e = 0; e < n_entries; ++e) {
        const uint32_t* row = entries + 5 * (size_t)e;
        const uint32_t p = row[0], off = row[1], cnt = row[2], mode = row[3], truth = row[4];
        if (p >= n_resid) return false;
        if (cnt < 1 || cnt > MG_AIM_MAX_PIECES) return false;
        if (off > n_pieces || cnt > n_pieces - off) return false;
        if (mode > MG_BOUND_HIGH_STRICT) return false;
        if (mode == MG_BOUND_XOR) {
            if (truth) return false;
            for (uint32_t k = 0; k < 8; ++k)
                if (fixed[8 * (size_t)e + k]) return false;
        } else if (truth & MG_BOUND_ATOM) {
            if ((truth & ~MG_BOUND_ATOM) >= n_atoms) return false;
        } else if (truth >= n_roots) {
            return false;
        }
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

/* the word of a base's mask state that holds an order entry's truth bit
 * (n_rwords: the words of the root mask rows) */
MG_AIM_FN uint32_t mg_walk_bound_truth_word(uint32_t truth, uint32_t n_rwords) {
    return truth & MG_BOUND_ATOM ? n_rwords + ((truth & ~MG_BOUND_ATOM) >> 5) : truth >> 5;
}

/* is entry e live: residual limb i at rvals[(p * 8 + i) * stride], mask word
 * i at mvals[i * stride] */
MG_AIM_FN bool mg_walk_bound_is_live(const uint32_t* entries, uint32_t e, const uint32_t* rvals,
                                     const uint32_t* mvals, uint32_t n_rwords, uint64_t stride) {
    const uint32_t p = entries[5 * (uint64_t)e], mode = entries[5 * (uint64_t)e + 3],
                   truth = entries[5 * (uint64_t)e + 4];
    if (mode != MG_BOUND_XOR)
        return !(mvals[(uint64_t)mg_walk_bound_truth_word(truth, n_rwords) * stride] >>
                 (truth & 31u) & 1u);
    uint32_t any = 0;
    for (uint32_t i = 0; i < 8; ++i) any |= rvals[((uint64_t)p * 8 + i) * stride];
    return any != 0;
}

/* Host only: L of a base with residual values rvals ([n_resid][8]) and mask
 * state mvals (NULL, either: round 0, nothing known) into live[1 ..], |L| into
 * live[0]. */
static inline void mg_walk_bound_live(const uint32_t* entries, uint32_t n_entries,
                                      const uint32_t* rvals, const uint32_t* mvals,
                                      uint32_t n_rwords, uint32_t* live) {
    uint32_t n = 0;
    for (uint32_t e = 0; rvals && mvals && e < n_entries; ++e)
        if (mg_walk_bound_is_live(entries, e, rvals, mvals, n_rwords, 1)) live[1 + n++] = e;
    live[0] = n;
}

/* a += b + carry (sub: a -= b + carry) mod 2^256: one fixed 8-limb chain */
MG_AIM_FN void mg_walk_bound_add(uint32_t* a, const uint32_t* b, uint32_t carry, bool sub) {
    for (uint32_t k = 0; k < 8; ++k) {
        if (!sub) {
            const uint64_t x = (uint64_t)a[k] + b[k] + carry;
            a[k] = (uint32_t)x;
            carry = (uint32_t)(x >> 32);
        } else {
            const uint64_t x = (uint64_t)a[k] - b[k] - carry;
            a[k] = (uint32_t)x;
            carry = (uint32_t)(x >> 63);
        }
    }
}

/* Lane j of round r applied to `dst` ([n_leaves][8] at dst[(leaf * 8 + k) *
 * stride], holding the base's values; dst may be the base itself): the pieces
 * of its entry applied, then its plain moves written over.  rvals: the base's
 * residual values ([n_resid][8]), live: its L.  *report and the return value
 * as mg_walk_aim_lane. */
MG_AIM_FN uint32_t mg_walk_bound_lane(const uint32_t* base, const mg_leafgen* gen,
                                      const uint32_t* consts, uint32_t n_leaves, uint64_t seed,
                                      uint32_t r, uint32_t j, uint32_t lanes,
                                      const uint32_t* entries, const uint32_t* pieces,
                                      const uint32_t* fixed, const uint32_t* rvals,
                                      const uint32_t* live, uint32_t* dst, uint64_t stride,
                                      mg_repair_moves* report) {
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
        const uint32_t p = entries[5 * (uint64_t)e], off = entries[5 * (uint64_t)e + 1],
                       cnt = entries[5 * (uint64_t)e + 2], mode = entries[5 * (uint64_t)e + 3];
        uint32_t t[8];
        for (uint32_t k = 0; k < 8; ++k) t[k] = rvals[(uint64_t)p * 8 + k];
        if (mode != MG_BOUND_XOR) {
            /* the side's value, gathered from the base before anything is
             * stored (dst may alias it), then the target T into t */
            uint32_t val[8];
            for (uint32_t k = 0; k < 8; ++k) val[k] = fixed[8 * (uint64_t)e + k];
            for (uint32_t q = off; q < off + cnt; ++q) {
                const uint32_t leaf = pieces[4 * (uint64_t)q];
                uint32_t v[8];
                for (uint32_t k = 0; k < 8; ++k) v[k] = base[(uint64_t)leaf * 8 + k];
                mg_walk_aim_shr(v, pieces[4 * (uint64_t)q + 1]);
                mg_repair_mask(v, pieces[4 * (uint64_t)q + 3]);
                mg_walk_aim_shl(v, pieces[4 * (uint64_t)q + 2]);
                for (uint32_t k = 0; k < 8; ++k) val[k] |= v[k];
            }
            const bool strict = mode == MG_BOUND_LOW_STRICT || mode == MG_BOUND_HIGH_STRICT;
            mg_walk_bound_add(val, t, strict ? 1u : 0u, mode <= MG_BOUND_LOW_STRICT);
            for (uint32_t k = 0; k < 8; ++k) t[k] = val[k];
        }
        for (uint32_t q = off; q < off + cnt; ++q) {
            const uint32_t leaf = pieces[4 * (uint64_t)q];
            if ((m0 && leaf0 == leaf) || (m1 && leaf1 == leaf)) continue;
            uint32_t v[8];
            for (uint32_t k = 0; k < 8; ++k) v[k] = t[k];
            mg_walk_aim_piece(v, pieces[4 * (uint64_t)q + 1], pieces[4 * (uint64_t)q + 2],
                              pieces[4 * (uint64_t)q + 3]);
            if (mode == MG_BOUND_XOR) {
                for (uint32_t k = 0; k < 8; ++k)
                    if (v[k]) dst[((uint64_t)leaf * 8 + k) * stride] ^= v[k];
            } else {
                uint32_t m[8];
                for (uint32_t k = 0; k < 8; ++k) m[k] = 0xFFFFFFFFu;
                mg_repair_mask(m, pieces[4 * (uint64_t)q + 3]);
                mg_walk_aim_shl(m, pieces[4 * (uint64_t)q + 1]);
                for (uint32_t k = 0; k < 8; ++k)
                    if (m[k]) {
                        uint32_t* d = dst + ((uint64_t)leaf * 8 + k) * stride;
                        *d = (*d & ~m[k]) | v[k];
                    }
            }
        }
    }
    if (m0)
        for (uint32_t k = 0; k < 8; ++k) dst[((uint64_t)leaf0 * 8 + k) * stride] = mv.val[0][k];
    if (m1)
        for (uint32_t k = 0; k < 8; ++k) dst[((uint64_t)leaf1 * 8 + k) * stride] = mv.val[1][k];
    return e;
}

#endif

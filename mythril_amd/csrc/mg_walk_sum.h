/* The aimed moves of mg_walk_sum, for host and device: the
 * lane function of mg_walk_uf.h whose entries may be linear.  The kernel that
 * writes the neighbours (mg_walk_sum_mutate), the kernel that adopts the best
 * one (mg_walk_sum_adopt) and the host entry the CPU suite compares with the
 * specification (mg_walk_sum_mutate_host) run the same code.  Specification,
 * bit for bit: mythril_amd/repair.py sum_mutate_ref.
 *
 * A linear entry belongs to a side S = sum of +-terms + numeral of a failing
 * atom, and its pieces are those of ONE term X of that sum (the target), not
 * of the side.  A move that changes only X by dX changes S by sign * dX mod
 * 2^w, so the entry gathers the target's value from the base as an order
 * entry of mg_walk_bound.h gathers its side,
 *   V = fixed | OR over pieces ((base[leaf] >> leaf_bit) & mask(len)) << value_bit
 * takes, with R / D the entry's residual probe and s = 1 for the strict modes,
 *   LOW, LOW_STRICT     d = D + s,          X = V - sign * d   (S := S - D - s)
 *   HIGH, HIGH_STRICT   d = D + s,          X = V + sign * d   (S := S + D + s)
 *   XOR                 d = (S xor R) - S,  X = V + sign * d   (S := S xor R)
 * all mod 2^256, and scatters X in piece order by masked overwrite, exactly
 * as an order entry scatters T (a leaf that a plain move of the lane owns is
 * skipped).  Only the XOR mode needs S, the side's own value under the base:
 * side row i is one 256-bit probe, written after the residual probes and
 * before the U rows, and the walker keeps the adopted lane's side rows.
 *   lin[e]   0: entry e is mg_walk_uf.h's.  Else
 *            bit 0      MG_SUM_LINEAR
 *            bit 1      MG_SUM_NEG: the target's sign in the side is -1
 *            bits 8-15  the side row (XOR mode; 0 in the order modes)
 *            every other bit 0
 * A linear XOR entry has truth 0 like every XOR entry, but its fixed value is
 * the target's numeral bits and may be set.  A linear entry has no slot piece.
 * The live rule, the lane layout and everything about entries that are not
 * linear are mg_walk_uf.h's: with lin all 0 so is every neighbour. */
#ifndef MG_WALK_SUM_H
#define MG_WALK_SUM_H

#include <stdint.h>
#include "mg_walk_uf.h"

#define MG_SUM_LINEAR 1u
#define MG_SUM_NEG 2u
#define MG_SUM_ROW_SHIFT 8u
#define MG_SUM_ROW_MASK 0xFFu
#define MG_SUM_MAX_ROWS 64u
#define MG_SUM_MAX_TERMS 4u

/* Everything mg_walk_uf_ok checks (a linear XOR entry may have fixed bits),
 * and: a known lin word per entry, the side row of a linear XOR entry below
 * n_srows <= 64 and 0 in a linear order entry, no slot piece in a linear
 * entry, no null lin with entries. */
static inline bool mg_walk_sum_ok(const uint32_t* entries, uint32_t n_entries,
                                  const uint32_t* pieces, uint32_t n_pieces,
                                  const uint32_t* fixed, const uint32_t* lin, uint32_t n_srows,
                                  const mg_leafgen* gen, uint32_t n_leaves, uint32_t n_resid,
                                  uint32_t n_roots, uint32_t n_atoms, const mg_uf_tables& t) {
    if (n_srows > MG_SUM_MAX_ROWS) return false;
    if (n_entries > MG_AIM_MAX_ENTRIES) return false;
    if (n_entries && (!entries || !fixed || !lin)) return false;
    if (n_pieces && !pieces) return false;
    bool linear_xor_fixed = false;
    for (uint32_t e = 0; e < n_entries; ++e) {
        const uint32_t lw = lin[e];
        if (!lw) continue;
        const uint32_t* row = entries + 5 * (size_t)e;
        const uint32_t off = row[1], cnt = row[2], mode = row[3];
        if (!(lw & MG_SUM_LINEAR)) return false;
        if (lw & ~(MG_SUM_LINEAR | MG_SUM_NEG | MG_SUM_ROW_MASK << MG_SUM_ROW_SHIFT)) return false;
        const uint32_t srow = lw >> MG_SUM_ROW_SHIFT & MG_SUM_ROW_MASK;
        if (mode == MG_BOUND_XOR ? srow >= n_srows : srow != 0) return false;
        if (off > n_pieces || cnt > n_pieces - off) return false;
        for (uint32_t q = off; q < off + cnt; ++q)
            if (pieces[4 * (size_t)q] & MG_UF_SLOT) return false;
        if (mode == MG_BOUND_XOR)
            for (uint32_t k = 0; k < 8; ++k)
                if (fixed[8 * (size_t)e + k]) linear_xor_fixed = true;
    }
    if (!linear_xor_fixed)
        return mg_walk_uf_ok(entries, n_entries, pieces, n_pieces, fixed, gen, n_leaves, n_resid,
                             n_roots, n_atoms, t);
    /* mg_walk_uf_ok refuses an XOR entry with a fixed word: the UF tables and
     * every entry but the linear XOR ones as they are, those with fixed 0 */
    uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!mg_walk_uf_ok(nullptr, 0, nullptr, 0, nullptr, gen, n_leaves, n_resid, n_roots, n_atoms, t))
        return false;
    for (uint32_t e = 0; e < n_entries; ++e) {
        const uint32_t* row = entries + 5 * (size_t)e;
        const bool lx = lin[e] && row[3] == MG_BOUND_XOR;
        /* one entry at a time, against the whole piece array */
        if (!mg_walk_uf_ok(row, 1, pieces, n_pieces, lx ? zero : fixed + 8 * (size_t)e, gen,
                           n_leaves, n_resid, n_roots, n_atoms, t))
            return false;
    }
    return true;
}

/* mg_walk_uf_lane with linear entries: lin ([n_entries]) and svals, the side
 * rows of the base ([n_srows][8]; read for a linear XOR entry alone). */
MG_AIM_FN uint32_t mg_walk_sum_lane(const uint32_t* base, const mg_leafgen* gen,
                                    const uint32_t* consts, uint32_t n_leaves, uint64_t seed,
                                    uint32_t r, uint32_t j, uint32_t lanes,
                                    const uint32_t* entries, const uint32_t* pieces,
                                    const uint32_t* fixed, const uint32_t* lin,
                                    const uint32_t* rvals, const uint32_t* svals,
                                    const uint32_t* live, const uint32_t* dest, uint32_t* dst,
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
        const uint32_t p = entries[5 * (uint64_t)e], off = entries[5 * (uint64_t)e + 1],
                       cnt = entries[5 * (uint64_t)e + 2], mode = entries[5 * (uint64_t)e + 3];
        const uint32_t lw = lin[e];
        const bool linear = (lw & MG_SUM_LINEAR) != 0;
        uint32_t t[8];
        for (uint32_t k = 0; k < 8; ++k) t[k] = rvals[(uint64_t)p * 8 + k];
        if (mode != MG_BOUND_XOR || linear) {
            /* the value of the side (of the target, when linear), gathered
             * from the base before anything is stored (dst may alias it),
             * then the value to scatter into t */
            uint32_t val[8];
            for (uint32_t k = 0; k < 8; ++k) val[k] = fixed[8 * (uint64_t)e + k];
            for (uint32_t q = off; q < off + cnt; ++q) {
                const uint32_t leaf = mg_walk_uf_leaf(pieces[4 * (uint64_t)q], dest);
                if (leaf >= n_leaves) continue;
                uint32_t v[8];
                for (uint32_t k = 0; k < 8; ++k) v[k] = base[(uint64_t)leaf * 8 + k];
                mg_walk_aim_shr(v, pieces[4 * (uint64_t)q + 1]);
                mg_repair_mask(v, pieces[4 * (uint64_t)q + 3]);
                mg_walk_aim_shl(v, pieces[4 * (uint64_t)q + 2]);
                for (uint32_t k = 0; k < 8; ++k) val[k] |= v[k];
            }
            const bool strict = mode == MG_BOUND_LOW_STRICT || mode == MG_BOUND_HIGH_STRICT;
            bool sub = mode == MG_BOUND_LOW || mode == MG_BOUND_LOW_STRICT;
            if (linear) {
                if (mode == MG_BOUND_XOR) {
                    /* d = (S xor R) - S */
                    const uint32_t* s = svals + (uint64_t)(lw >> MG_SUM_ROW_SHIFT & MG_SUM_ROW_MASK) * 8;
                    uint32_t sv[8];
                    for (uint32_t k = 0; k < 8; ++k) {
                        sv[k] = s[k];
                        t[k] ^= sv[k];
                    }
                    mg_walk_bound_add(t, sv, 0u, true);
                }
                if (lw & MG_SUM_NEG) sub = !sub;
            }
            mg_walk_bound_add(val, t, strict ? 1u : 0u, sub);
            for (uint32_t k = 0; k < 8; ++k) t[k] = val[k];
        }
        for (uint32_t q = off; q < off + cnt; ++q) {
            const uint32_t leaf = mg_walk_uf_leaf(pieces[4 * (uint64_t)q], dest);
            if (leaf >= n_leaves) continue;
            if ((m0 && leaf0 == leaf) || (m1 && leaf1 == leaf)) continue;
            uint32_t v[8];
            for (uint32_t k = 0; k < 8; ++k) v[k] = t[k];
            mg_walk_aim_piece(v, pieces[4 * (uint64_t)q + 1], pieces[4 * (uint64_t)q + 2],
                              pieces[4 * (uint64_t)q + 3]);
            if (mode == MG_BOUND_XOR && !linear) {
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

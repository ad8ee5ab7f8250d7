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
 * linear are mg_walk_uf.h's: with lin all 0 so is every neighbour.
 *
 * The three rungs are nested, so this header holds the code of all three once:
 * mg_walk_sum_lane is the lane function, mg_walk_uf_ok the entry validator and
 * mg_walk_uf_live the live rule; the uf rung is the sum rung with lin words
 * all 0 (mg_walk_no_lin on the host, a zeroed array on the device) and the
 * bound rung is the uf rung with empty UF tables and no destinations.
 * mg_walk_bound.h and mg_walk_uf.h describe their rung's tables and include
 * this file. */
#ifndef MG_WALK_SUM_H
#define MG_WALK_SUM_H

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

#define MG_UF_SLOT 0x80000000u
#define MG_UF_MAX_SLOTS 64u
#define MG_UF_MAX_FUNCS 64u
#define MG_UF_MAX_CANDS 256u
#define MG_UF_MAX_ROWS 128u
#define MG_UF_MAX_CHUNKS 4u
#define MG_UF_CONST 0u
#define MG_UF_LEAF 1u
#define MG_UF_PROBE 2u
#define MG_UF_ALWAYS 3u

/* the UF tables of one walk */
struct mg_uf_tables {
    const uint32_t* slots;
    uint32_t n_slots;
    const uint32_t* funcs;
    uint32_t n_funcs;
    const uint32_t* cands;
    uint32_t n_cands;
    const uint32_t* ukeys;
    uint32_t n_ukeys;
    uint32_t n_urows;
};

#define MG_SUM_LINEAR 1u
#define MG_SUM_NEG 2u
#define MG_SUM_ROW_SHIFT 8u
#define MG_SUM_ROW_MASK 0xFFu
#define MG_SUM_MAX_ROWS 64u
#define MG_SUM_MAX_TERMS 4u

/* the lin words of a table with no linear entry (host) */
static const uint32_t mg_walk_no_lin[MG_AIM_MAX_ENTRIES] = {0};

/* The width of function f's value leaves: 0 when it has none, MG_AIM_NONE
 * when two differ or one is wider than 256 bits.  The candidates must be in
 * range. */
static inline uint32_t mg_walk_uf_width(const mg_uf_tables& t, uint32_t f, const mg_leafgen* gen) {
    uint32_t w = 0;
    const uint32_t first = t.funcs[3 * (size_t)f], cnt = t.funcs[3 * (size_t)f + 1];
    for (uint32_t c = first; c < first + cnt; ++c) {
        const uint32_t leaf = t.cands[6 * (size_t)c];
        if (leaf == MG_AIM_NONE) continue;
        const uint32_t lw = gen[leaf].width;
        if (lw < 1 || lw > 256 || (w && lw != w)) return MG_AIM_NONE;
        w = lw;
    }
    return w;
}

/* Everything mg_walk_aim_ok checks, and: mode <= 4, the truth index below
 * n_atoms, respectively n_roots, truth and fixed zero for XOR entries.  For
 * slot pieces and the UF tables: slot, function, candidate and U-row indices
 * in range, 1 .. 4 chunks, key words in range for their kind, one width for
 * the value leaves of a function, each slot piece inside that width, no
 * argument or PROBE row at or past n_urows, no null pointer with a count. */
static inline bool mg_walk_uf_ok(const uint32_t* entries, uint32_t n_entries,
                                 const uint32_t* pieces, uint32_t n_pieces,
                                 const uint32_t* fixed, const mg_leafgen* gen, uint32_t n_leaves,
                                 uint32_t n_resid, uint32_t n_roots, uint32_t n_atoms,
                                 const mg_uf_tables& t) {
    if (t.n_slots > MG_UF_MAX_SLOTS || t.n_funcs > MG_UF_MAX_FUNCS ||
        t.n_cands > MG_UF_MAX_CANDS || t.n_urows > MG_UF_MAX_ROWS)
        return false;
    if ((t.n_slots && !t.slots) || (t.n_funcs && !t.funcs) || (t.n_cands && !t.cands) ||
        (t.n_ukeys && !t.ukeys))
        return false;
    if ((t.n_slots || t.n_funcs) && !gen) return false;
    for (uint32_t f = 0; f < t.n_funcs; ++f) {
        const uint32_t first = t.funcs[3 * (size_t)f], cnt = t.funcs[3 * (size_t)f + 1],
                       chunks = t.funcs[3 * (size_t)f + 2];
        if (chunks < 1 || chunks > MG_UF_MAX_CHUNKS) return false;
        if (first > t.n_cands || cnt > t.n_cands - first) return false;
        for (uint32_t c = first; c < first + cnt; ++c) {
            const uint32_t* row = t.cands + 6 * (size_t)c;
            if (row[0] != MG_AIM_NONE && row[0] >= n_leaves) return false;
            if (row[1] > MG_UF_ALWAYS) return false;
            for (uint32_t k = 0; k < chunks; ++k) {
                const uint32_t key = row[2 + k];
                if (row[1] == MG_UF_CONST && key >= t.n_ukeys) return false;
                if (row[1] == MG_UF_LEAF && key >= n_leaves) return false;
                if (row[1] == MG_UF_PROBE && key >= t.n_urows) return false;
            }
        }
        if (mg_walk_uf_width(t, f, gen) == MG_AIM_NONE) return false;
    }
    for (uint32_t u = 0; u < t.n_slots; ++u) {
        const uint32_t f = t.slots[2 * (size_t)u], row = t.slots[2 * (size_t)u + 1];
        if (f >= t.n_funcs) return false;
        const uint32_t chunks = t.funcs[3 * (size_t)f + 2];
        if (row > t.n_urows || chunks > t.n_urows - row) return false;
    }
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
            uint32_t w;
            if (leaf & MG_UF_SLOT) {
                const uint32_t u = leaf & ~MG_UF_SLOT;
                if (u >= t.n_slots) return false;
                w = mg_walk_uf_width(t, t.slots[2 * (size_t)u], gen);
            } else {
                if (leaf >= n_leaves) return false;
                w = gen[leaf].width;
            }
            if (w > 256 || len < 1 || len > 256) return false;
            if (leaf_bit > w || len > w - leaf_bit) return false;
            if (value_bit > 256 || len > 256 - value_bit) return false;
        }
    }
    return true;
}

/* mg_walk_uf_ok with empty UF tables: a piece with the slot bit names no slot
 * and is refused, as a leaf index at or above n_leaves is. */
static inline bool mg_walk_bound_ok(const uint32_t* entries, uint32_t n_entries,
                                    const uint32_t* pieces, uint32_t n_pieces,
                                    const uint32_t* fixed, const mg_leafgen* gen,
                                    uint32_t n_leaves, uint32_t n_resid, uint32_t n_roots,
                                    uint32_t n_atoms) {
    const mg_uf_tables none = {nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, 0};
    return mg_walk_uf_ok(entries, n_entries, pieces, n_pieces, fixed, gen, n_leaves, n_resid,
                         n_roots, n_atoms, none);
}

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

/* The destination of slot u: base ([n_leaves][8]) is the adopted base, U row
 * i's limb k at urows[(i * 8 + k) * stride]. */
MG_AIM_FN uint32_t mg_walk_uf_resolve(const uint32_t* slots, const uint32_t* funcs,
                                      const uint32_t* cands, const uint32_t* ukeys, uint32_t u,
                                      const uint32_t* base, const uint32_t* urows,
                                      uint64_t stride) {
    const uint32_t f = slots[2 * (uint64_t)u], arg = slots[2 * (uint64_t)u + 1];
    const uint32_t first = funcs[3 * (uint64_t)f], cnt = funcs[3 * (uint64_t)f + 1],
                   chunks = funcs[3 * (uint64_t)f + 2];
    for (uint32_t c = first; c < first + cnt; ++c) {
        const uint32_t* row = cands + 6 * (uint64_t)c;
        const uint32_t kind = row[1];
        uint32_t differ = 0;
        for (uint32_t k = 0; kind != MG_UF_ALWAYS && k < chunks; ++k) {
            const uint32_t key = row[2 + k];
            for (uint32_t i = 0; i < 8; ++i) {
                const uint32_t a = urows[(((uint64_t)arg + k) * 8 + i) * stride];
                const uint32_t b = kind == MG_UF_CONST ? ukeys[(uint64_t)key * 8 + i]
                                   : kind == MG_UF_LEAF ? base[(uint64_t)key * 8 + i]
                                                        : urows[((uint64_t)key * 8 + i) * stride];
                differ |= a ^ b;
            }
        }
        if (!differ) return row[0];
    }
    return MG_AIM_NONE;
}

/* is entry e live: mg_walk_bound_is_live, and no slot piece of it has the
 * destination MG_AIM_NONE (dest: the walker's n_slots destinations; NULL: the
 * table has no slot piece, and pieces is not read) */
MG_AIM_FN bool mg_walk_uf_is_live(const uint32_t* entries, const uint32_t* pieces, uint32_t e,
                                  const uint32_t* rvals, const uint32_t* mvals, uint32_t n_rwords,
                                  uint64_t stride, const uint32_t* dest) {
    if (!mg_walk_bound_is_live(entries, e, rvals, mvals, n_rwords, stride)) return false;
    if (!dest) return true;
    const uint32_t off = entries[5 * (uint64_t)e + 1], cnt = entries[5 * (uint64_t)e + 2];
    for (uint32_t q = off; q < off + cnt; ++q) {
        const uint32_t leaf = pieces[4 * (uint64_t)q];
        if ((leaf & MG_UF_SLOT) && dest[leaf & ~MG_UF_SLOT] == MG_AIM_NONE) return false;
    }
    return true;
}

/* Host only: L of a base with residual values rvals ([n_resid][8]) and mask
 * state mvals (NULL, either: round 0, nothing known) into live[1 ..], |L| into
 * live[0]; dest may be NULL when the table has no slot. */
static inline void mg_walk_uf_live(const uint32_t* entries, uint32_t n_entries,
                                   const uint32_t* pieces, const uint32_t* rvals,
                                   const uint32_t* mvals, uint32_t n_rwords, const uint32_t* dest,
                                   uint32_t* live) {
    uint32_t n = 0;
    for (uint32_t e = 0; rvals && mvals && e < n_entries; ++e)
        if (mg_walk_uf_is_live(entries, pieces, e, rvals, mvals, n_rwords, 1, dest))
            live[1 + n++] = e;
    live[0] = n;
}

/* mg_walk_uf_live with no destinations */
static inline void mg_walk_bound_live(const uint32_t* entries, uint32_t n_entries,
                                      const uint32_t* rvals, const uint32_t* mvals,
                                      uint32_t n_rwords, uint32_t* live) {
    mg_walk_uf_live(entries, n_entries, nullptr, rvals, mvals, n_rwords, nullptr, live);
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

/* the leaf a piece acts on: its own, or its slot's destination */
MG_AIM_FN uint32_t mg_walk_uf_leaf(uint32_t leaf, const uint32_t* dest) {
    return leaf & MG_UF_SLOT ? dest[leaf & ~MG_UF_SLOT] : leaf;
}

/* Lane j of round r applied to `dst` ([n_leaves][8] at dst[(leaf * 8 + k) *
 * stride], holding the base's values; dst may be the base itself): the pieces
 * of its entry applied, then its plain moves written over.  rvals: the base's
 * residual values ([n_resid][8]), live: its L, dest: the walker's destinations
 * (read for a slot piece alone), lin ([n_entries]) and
 * svals, the side rows of the base ([n_srows][8]; read for a linear XOR entry
 * alone).  *report and the return value as mg_walk_aim_lane.  (A live entry
 * has no unresolved slot piece; a piece whose leaf is not below n_leaves is
 * skipped all the same.) */
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

/* Host only (the kernels call mg_walk_sum_lane): the uf rung, no linear entry
 * and so no side row */
static inline uint32_t mg_walk_uf_lane(const uint32_t* base, const mg_leafgen* gen,
                                   const uint32_t* consts, uint32_t n_leaves, uint64_t seed,
                                   uint32_t r, uint32_t j, uint32_t lanes,
                                   const uint32_t* entries, const uint32_t* pieces,
                                   const uint32_t* fixed, const uint32_t* rvals,
                                   const uint32_t* live, const uint32_t* dest, uint32_t* dst,
                                   uint64_t stride, mg_repair_moves* report) {
    return mg_walk_sum_lane(base, gen, consts, n_leaves, seed, r, j, lanes, entries, pieces, fixed,
                            mg_walk_no_lin, rvals, nullptr, live, dest, dst, stride, report);
}

/* Host only: the bound rung, no slot piece either and so no destinations */
static inline uint32_t mg_walk_bound_lane(const uint32_t* base, const mg_leafgen* gen,
                                      const uint32_t* consts, uint32_t n_leaves, uint64_t seed,
                                      uint32_t r, uint32_t j, uint32_t lanes,
                                      const uint32_t* entries, const uint32_t* pieces,
                                      const uint32_t* fixed, const uint32_t* rvals,
                                      const uint32_t* live, uint32_t* dst, uint64_t stride,
                                      mg_repair_moves* report) {
    return mg_walk_uf_lane(base, gen, consts, n_leaves, seed, r, j, lanes, entries, pieces, fixed,
                           rvals, live, nullptr, dst, stride, report);
}


#endif

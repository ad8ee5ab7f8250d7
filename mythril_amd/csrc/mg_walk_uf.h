/* The aimed moves of mg_walk_uf, for host and device: the
 * lane function of mg_walk_bound.h whose pieces may name a UF slot instead of
 * a leaf.  The kernel that writes the neighbours (mg_walk_uf_mutate), the
 * kernel that adopts the best one and resolves the slots (mg_walk_uf_adopt)
 * and the host entries the CPU suite compares with the specification
 * (mg_walk_uf_mutate_host, mg_walk_uf_resolve_host) run the same code.
 * Specification, bit for bit: mythril_amd/repair.py uf_resolve_ref,
 * uf_mutate_ref.
 *
 * A slot is one application f(arg) of an uninterpreted function.  Its value
 * is whichever entry of f's model table arg hits under the current
 * assignment, so the leaf an aim writes is resolved per walker, at every
 * adoption, from the adopted base and the adopted lane's U rows (the probes
 * after the residuals: the arguments' chunks, then the computed keys of
 * argument-keyed entries):
 *   slots[2 u ..]   function, first U row of the argument (one per key chunk)
 *   funcs[3 f ..]   first candidate, candidates, key chunks (1 .. 4)
 *   cands[6 c ..]   value leaf or MG_AIM_NONE, key kind, key word per chunk
 *   ukeys[8 n ..]   the chunks of the constant keys
 *   key kind        0 CONST: a row of ukeys; 1 LEAF: a leaf; 2 PROBE: a U row;
 *                   3 ALWAYS: no key, matches (the else leaf)
 * The candidates of a function stand in the table's precedence order.  The
 * destination of slot u is the value leaf of the FIRST candidate of its
 * function all of whose key chunks equal the argument's U rows in all 8 limbs
 * (MG_AIM_NONE when none matches or that candidate has no value leaf).
 *
 *   pieces[4 p ..]  MG_UF_SLOT | u, leaf_bit, value_bit, len: acts on leaf
 *                   dest[u] wherever mg_walk_bound.h says leaf
 * An entry with a slot piece whose destination is MG_AIM_NONE is not live;
 * everything else (entries, fixed, modes, truth, L, the lane layout) is
 * mg_walk_bound.h's, and with no slot piece so is every neighbour. */
#ifndef MG_WALK_UF_H
#define MG_WALK_UF_H

#include <stdint.h>
#include "mg_walk_bound.h"

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

/* Everything mg_walk_bound_ok checks for leaf pieces, and for slot pieces and
 * the UF tables: slot, function, candidate and U-row indices in range, 1 .. 4
 * chunks, key words in range for their kind, one width for the value leaves
 * of a function, each slot piece inside that width, no argument or PROBE row
 * at or past n_urows, no null pointer with a count. */
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
 * destination MG_AIM_NONE (dest: the walker's n_slots destinations) */
MG_AIM_FN bool mg_walk_uf_is_live(const uint32_t* entries, const uint32_t* pieces, uint32_t e,
                                  const uint32_t* rvals, const uint32_t* mvals, uint32_t n_rwords,
                                  uint64_t stride, const uint32_t* dest) {
    if (!mg_walk_bound_is_live(entries, e, rvals, mvals, n_rwords, stride)) return false;
    const uint32_t off = entries[5 * (uint64_t)e + 1], cnt = entries[5 * (uint64_t)e + 2];
    for (uint32_t q = off; q < off + cnt; ++q) {
        const uint32_t leaf = pieces[4 * (uint64_t)q];
        if ((leaf & MG_UF_SLOT) && dest[leaf & ~MG_UF_SLOT] == MG_AIM_NONE) return false;
    }
    return true;
}

/* Host only: L into live[1 ..], |L| into live[0] (as mg_walk_bound_live; dest
 * may be NULL when the table has no slot). */
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

/* the leaf a piece acts on: its own, or its slot's destination */
MG_AIM_FN uint32_t mg_walk_uf_leaf(uint32_t leaf, const uint32_t* dest) {
    return leaf & MG_UF_SLOT ? dest[leaf & ~MG_UF_SLOT] : leaf;
}

/* mg_walk_bound_lane with slot pieces: dest holds the walker's destinations.
 * (A live entry has no unresolved slot piece; a piece whose leaf is not below
 * n_leaves is skipped all the same.) */
MG_AIM_FN uint32_t mg_walk_uf_lane(const uint32_t* base, const mg_leafgen* gen,
                                   const uint32_t* consts, uint32_t n_leaves, uint64_t seed,
                                   uint32_t r, uint32_t j, uint32_t lanes,
                                   const uint32_t* entries, const uint32_t* pieces,
                                   const uint32_t* fixed, const uint32_t* rvals,
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
        uint32_t t[8];
        for (uint32_t k = 0; k < 8; ++k) t[k] = rvals[(uint64_t)p * 8 + k];
        if (mode != MG_BOUND_XOR) {
            /* the side's value, gathered from the base before anything is
             * stored (dst may alias it), then the target T into t */
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
            mg_walk_bound_add(val, t, strict ? 1u : 0u, mode <= MG_BOUND_LOW_STRICT);
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

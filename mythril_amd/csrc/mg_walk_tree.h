/* The tree scoring of the scored walk (mg_walk_tree), for
 * host and device: a failing root's cost is the branch distance of a small
 * postfix program over atoms — and = sum, or = minimum — so a root made of
 * equalities and orders under and/or/ite/store chains has a gradient.  The
 * kernel (mg_walk_tree_score) and the host entry (mg_walk_tree_score_host)
 * run the same code.  Specification, bit for bit: mythril_amd/repair.py
 * tree_score_ref; the tables are built by repair.py distance_trees.
 *
 * Probes of the program, in order: [root mask | atom mask | residuals].
 *   roots[k]   a simple entry kind << 16 | residual probe (exactly a table
 *              entry of mg_walk.h), or MG_WT_TREE | offset of the root's
 *              program in code
 *   atoms[i]   kind << 16 | residual probe: atom i holds when bit i of the
 *              atom mask is set; when it does not it is d_i away, the
 *              distances of mg_walk.h (1, max(1, popcount R), 1 + bitlen R)
 *   code       u32 words op << 16 | argument:
 *                ATOM i  push 0 if atom i holds, else d_i
 *                AND n   pop n, push their sum saturating at MG_WT_INF
 *                OR n    pop n, push their minimum
 *                INF     push MG_WT_INF
 *                END     the top is the root's value
 * A failing tree root costs clamp(top, 1, MG_WT_INF); cost is the sum over
 * the failing roots, at most 1024 * 1023 < 2^20.  Whether a root holds is
 * read from its root mask bit alone. */
#ifndef MG_WALK_TREE_H
#define MG_WALK_TREE_H

#include <stdint.h>
#include "mg_walk.h"

#define MG_WT_TREE 0x80000000u
#define MG_WT_END 0u
#define MG_WT_ATOM 1u
#define MG_WT_AND 2u
#define MG_WT_OR 3u
#define MG_WT_PUSH_INF 4u
#define MG_WT_OPS 5u
#define MG_WT_INF 1023u
#define MG_WT_MAX_ROOTS 1024u
#define MG_WT_MAX_ATOMS 1024u        /* in all */
#define MG_WT_ROOT_ATOMS 32u         /* ATOM words of one root's program */
#define MG_WT_ROOT_WORDS 64u         /* words of one root's program, END included */
#define MG_WT_STACK 8u
#define MG_WT_MAX_CODE (MG_WT_MAX_ROOTS * MG_WT_ROOT_WORDS)

/* a table entry (of a simple root or of an atom) names a known kind and,
 * unless flat, a residual probe there is */
MG_WALK_FN bool mg_walk_tree_entry_ok(uint32_t entry, uint32_t n_resid) {
    const uint32_t kind = entry >> 16, p = entry & 0xFFFFu;
    return kind < MG_WALK_KINDS && (kind == MG_WALK_FLAT || p < n_resid);
}

/* The validator: every table entry as above; every tree root's offset inside
 * code; its program made of known words over atoms below n_atoms, at most
 * MG_WT_ROOT_ATOMS of them, the stack never underflowing and never deeper
 * than MG_WT_STACK, END within MG_WT_ROOT_WORDS words and inside code, with
 * exactly one value on the stack.  A table it accepts makes
 * mg_walk_tree_score_lane read inside the tables, the atom mask and the
 * residual probes. */
MG_WALK_FN bool mg_walk_tree_ok(const uint32_t* roots, uint32_t n_roots, const uint32_t* atoms,
                                uint32_t n_atoms, const uint32_t* code, uint32_t n_code,
                                uint32_t n_resid) {
    if (n_roots < 1 || n_roots > MG_WT_MAX_ROOTS || n_atoms > MG_WT_MAX_ATOMS ||
        n_code > MG_WT_MAX_CODE || n_resid > 0xFFFFu)
        return false;
    if (!roots || (n_atoms && !atoms) || (n_code && !code)) return false;
    for (uint32_t i = 0; i < n_atoms; ++i)
        if (!mg_walk_tree_entry_ok(atoms[i], n_resid)) return false;
    for (uint32_t k = 0; k < n_roots; ++k) {
        if (!(roots[k] & MG_WT_TREE)) {
            if (!mg_walk_tree_entry_ok(roots[k], n_resid)) return false;
            continue;
        }
        const uint32_t off = roots[k] & ~MG_WT_TREE;
        if (off >= n_code) return false;
        uint32_t depth = 0, n_atom_words = 0, pc = off;
        for (;; ++pc) {
            if (pc >= n_code || pc - off >= MG_WT_ROOT_WORDS) return false;
            const uint32_t op = code[pc] >> 16, arg = code[pc] & 0xFFFFu;
            if (op == MG_WT_END) {
                if (arg != 0 || depth != 1) return false;
                break;
            }
            if (op == MG_WT_ATOM) {
                if (arg >= n_atoms || ++n_atom_words > MG_WT_ROOT_ATOMS) return false;
                ++depth;
            } else if (op == MG_WT_PUSH_INF) {
                if (arg != 0) return false;
                ++depth;
            } else if (op == MG_WT_AND || op == MG_WT_OR) {
                if (arg < 1 || arg > depth) return false;
                depth -= arg - 1;
            } else {
                return false;
            }
            if (depth > MG_WT_STACK) return false;
        }
    }
    return true;
}

/* the distance of a residual: limb i of probe p at resid[(p * 8 + i) * stride + col] */
MG_WALK_FN uint32_t mg_walk_tree_resid(const uint32_t* resid, uint64_t stride, uint64_t col,
                                       uint32_t kind, uint32_t p) {
    uint32_t pop = 0, len = 0;
    for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t limb = resid[((uint64_t)p * 8 + i) * stride + col];
        pop += mg_walk_popc(limb);
        if (limb) len = 32 * i + 32 - mg_walk_clz(limb);
    }
    return kind == MG_WALK_HAMMING ? (pop ? pop : 1u) : 1u + len;
}

/* (nfail, cost) of lane `col`, as mg_walk_score_lane: masks, amasks: the
 * rows of the root mask and of the atom mask (word q of the lane at
 * [q * stride + col]), resid: the residual probes.  stack: MG_WT_STACK words
 * of this lane, level d at stack[d * sstride] (LDS on the device: the stack
 * pointer is wave-uniform but dynamic).  The tables must have passed
 * mg_walk_tree_ok.  Per 32 roots the wave-wide OR of the failing bits selects
 * the roots some lane fails; a tree root's program is wave-uniform, every
 * lane of the wave runs it and a lane that does not fail the root adds 0.
 * An atom's word is read by the lanes that fail the root, a residual's eight
 * limb rows by those whose atom is false besides. */
MG_WALK_FN void mg_walk_tree_score_lane(const uint32_t* masks, const uint32_t* amasks,
                                        const uint32_t* resid, uint64_t stride, uint64_t col,
                                        const uint32_t* roots, const uint32_t* atoms,
                                        const uint32_t* code, uint32_t n_roots, bool active,
                                        uint32_t* stack, uint32_t sstride, uint32_t* out_nfail,
                                        uint32_t* out_cost) {
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
            const uint32_t entry = roots[32 * q + b];                  /* wave-uniform load */
            const bool f = (fails >> b & 1u) != 0;
            if (!(entry & MG_WT_TREE)) {                               /* simple: as mg_walk.h */
                const uint32_t kind = entry >> 16, p = entry & 0xFFFFu;
                if (kind == MG_WALK_FLAT)
                    cost += f ? 1u : 0u;
                else if (f)
                    cost += mg_walk_tree_resid(resid, stride, col, kind, p);
                continue;
            }
            uint32_t sp = 0;                                           /* wave-uniform */
            for (uint32_t pc = entry & ~MG_WT_TREE;; ++pc) {
                const uint32_t word = code[pc];                        /* wave-uniform load */
                const uint32_t op = word >> 16, arg = word & 0xFFFFu;
                if (op == MG_WT_END) break;
                if (op == MG_WT_ATOM) {
                    const uint32_t a = atoms[arg];                     /* wave-uniform load */
                    uint32_t d = 0;
                    if (f && !(amasks[(uint64_t)(arg >> 5) * stride + col] >> (arg & 31u) & 1u)) {
                        const uint32_t kind = a >> 16;
                        d = kind == MG_WALK_FLAT
                                ? 1u
                                : mg_walk_tree_resid(resid, stride, col, kind, a & 0xFFFFu);
                    }
                    stack[sp++ * sstride] = d;
                } else if (op == MG_WT_PUSH_INF) {
                    stack[sp++ * sstride] = MG_WT_INF;
                } else {
                    uint32_t v = stack[(sp - 1) * sstride];
                    for (uint32_t i = 2; i <= arg; ++i) {
                        const uint32_t o = stack[(sp - i) * sstride];
                        v = op == MG_WT_AND ? v + o : (o < v ? o : v);
                        v = v > MG_WT_INF ? MG_WT_INF : v;
                    }
                    sp -= arg - 1;
                    stack[(sp - 1) * sstride] = v;
                }
            }
            const uint32_t top = stack[0];
            cost += f ? (top < 1u ? 1u : (top > MG_WT_INF ? MG_WT_INF : top)) : 0u;
        }
    }
    *out_nfail = nfail;
    *out_cost = cost;
}

#endif

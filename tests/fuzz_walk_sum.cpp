// Sanitizer fuzz of the safety boundary of the aims through sums (DESIGN.md
// §3.15): csrc/mg_walk_sum.h alone.  Random valid tables (XOR and order
// entries, linear or not, with leaf and slot pieces, UF tables with every key
// kind, side rows), mutated copies and random words go through the validator
// (mg_walk_sum_ok); whatever it accepts is run through the resolver, the live
// list and the lane function (mg_walk_sum_lane) on buffers allocated at
// exactly the sizes the accepted counts imply, so a read or write outside a
// table, the lin words, the side rows, the U rows, the destinations or the
// leaves is an ASan report, and a neighbour with a bit beyond a leaf's width
// aborts.  Every third run applies the lane to the base itself, as the adopt
// kernel does, and must give what a separate destination gives.  Stand-alone:
// its own main, built with g++ -fsanitize=address,undefined
// (tests/test_walk_sum_sanitize.py).
//
//   fuzz_walk_sum [iterations]   prints one JSON line of counters

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mg_walk_sum.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}
static uint32_t below(uint32_t n) { return n ? rnd() % n : 0; }

struct Tables {
    std::vector<mg_leafgen> gen;
    std::vector<uint32_t> entries, pieces, fixed, lin, slots, funcs, cands, ukeys;
    uint32_t n_resid = 0, n_roots = 0, n_atoms = 0, n_urows = 0, n_srows = 0;
};

static Tables valid() {
    Tables t;
    const uint32_t widths[] = {1, 7, 8, 13, 31, 32, 33, 64, 100, 143, 160, 255, 256};
    // the functions first: each owns a run of leaves of one width (its values)
    const uint32_t n_funcs = below(4) == 0 ? 0 : 1 + below(below(6) ? 4 : MG_UF_MAX_FUNCS);
    std::vector<std::vector<uint32_t>> values(n_funcs);
    std::vector<uint32_t> fwidth(n_funcs);
    for (uint32_t f = 0; f < n_funcs; ++f) {
        fwidth[f] = below(3) ? widths[below(13)] : 1 + below(256);
        for (uint32_t i = 0, n = 1 + below(4); i < n; ++i) {
            mg_leafgen g;
            memset(&g, 0, sizeof g);
            g.width = fwidth[f];
            values[f].push_back((uint32_t)t.gen.size());
            t.gen.push_back(g);
        }
    }
    const uint32_t n_plain = 1 + below(below(4) ? 12 : 40);
    for (uint32_t i = 0; i < n_plain; ++i) {
        mg_leafgen g;
        memset(&g, 0, sizeof g);
        g.width = below(3) ? widths[below(13)] : 1 + below(256);
        t.gen.push_back(g);
    }
    const uint32_t n_leaves = (uint32_t)t.gen.size();
    t.n_urows = n_funcs ? 4 + below(below(4) ? 12 : MG_UF_MAX_ROWS - 3) : below(3);
    for (uint32_t i = 0, n = below(5); i < n * 8; ++i) t.ukeys.push_back(below(2) ? below(4) : rnd());
    const uint32_t n_ukeys = (uint32_t)t.ukeys.size() / 8;
    for (uint32_t f = 0; f < n_funcs; ++f) {
        const uint32_t chunks = 1 + below(MG_UF_MAX_CHUNKS);
        uint32_t cnt = 1 + below(below(8) ? 4 : 12);
        if (t.cands.size() / 6 + cnt > MG_UF_MAX_CANDS) cnt = 0;
        t.funcs.insert(t.funcs.end(), {(uint32_t)t.cands.size() / 6, cnt, chunks});
        for (uint32_t c = 0; c < cnt; ++c) {
            uint32_t kind = below(4);
            if (kind == MG_UF_CONST && !n_ukeys) kind = MG_UF_ALWAYS;
            t.cands.push_back(below(4) == 0 ? MG_AIM_NONE
                                            : values[f][below((uint32_t)values[f].size())]);
            t.cands.push_back(kind);
            for (uint32_t k = 0; k < MG_UF_MAX_CHUNKS; ++k)
                t.cands.push_back(k >= chunks ? rnd()            // never read
                                  : kind == MG_UF_CONST ? below(n_ukeys)
                                  : kind == MG_UF_LEAF ? below(n_leaves)
                                  : kind == MG_UF_PROBE ? below(t.n_urows) : rnd());
        }
    }
    const uint32_t n_slots = n_funcs ? below(below(6) ? 6 : MG_UF_MAX_SLOTS + 1) : 0;
    std::vector<uint32_t> usable;                        // slots whose function has a value leaf
    for (uint32_t u = 0; u < n_slots; ++u) {
        const uint32_t f = below(n_funcs), chunks = t.funcs[3 * f + 2];
        t.slots.insert(t.slots.end(), {f, below(t.n_urows - chunks + 1)});
        bool any = false;
        for (uint32_t c = t.funcs[3 * f]; c < t.funcs[3 * f] + t.funcs[3 * f + 1]; ++c)
            any = any || t.cands[6 * c] != MG_AIM_NONE;
        if (any) usable.push_back(u);
    }
    t.n_resid = 1 + below(12);
    t.n_srows = below(4) ? 1 + below(below(4) ? 6 : MG_SUM_MAX_ROWS) : 0;
    t.n_roots = 1 + below(below(3) ? 40 : 1024);
    t.n_atoms = below(below(3) ? 70 : 1025);
    const uint32_t n_entries = below(8) == 0 ? MG_AIM_MAX_ENTRIES - below(2) : below(12);
    for (uint32_t e = 0; e < n_entries; ++e) {
        const uint32_t cnt = below(6) == 0 ? MG_AIM_MAX_PIECES : 1 + below(8);
        t.entries.push_back(below(t.n_resid));
        t.entries.push_back((uint32_t)t.pieces.size() / 4);
        t.entries.push_back(cnt);
        const uint32_t mode = below(5);
        // linear: every mode, both signs; an XOR one needs a side row
        const bool linear = below(2) && (mode != MG_BOUND_XOR || t.n_srows);
        t.lin.push_back(!linear ? 0u : MG_SUM_LINEAR | (below(2) ? MG_SUM_NEG : 0u) |
                        (mode == MG_BOUND_XOR ? below(t.n_srows) << MG_SUM_ROW_SHIFT : 0u));
        t.entries.push_back(mode);
        t.entries.push_back(mode == MG_BOUND_XOR ? 0u :
                            t.n_atoms && below(2) ? MG_BOUND_ATOM | below(t.n_atoms)
                                                  : below(t.n_roots));
        for (uint32_t k = 0; k < 8; ++k)
            t.fixed.push_back((mode == MG_BOUND_XOR && !linear) || below(3) == 0
                                  ? 0u : rnd() ^ rnd() << 16);
        for (uint32_t q = 0; q < cnt; ++q) {
            uint32_t leaf = below(n_leaves), w = t.gen[leaf].width;
            if (!linear && !usable.empty() && below(3) == 0) {
                const uint32_t u = usable[below((uint32_t)usable.size())];
                leaf = MG_UF_SLOT | u;
                w = fwidth[t.slots[2 * u]];
            }
            const uint32_t len = 1 + below(w), leaf_bit = below(w - len + 1),
                           value_bit = below(256 - len + 1);
            t.pieces.insert(t.pieces.end(), {leaf, leaf_bit, value_bit, len});
        }
    }
    return t;
}

static void mutate(Tables& t) {
    const uint32_t n = 1 + below(3);
    for (uint32_t i = 0; i < n; ++i) {
        std::vector<uint32_t>* all[] = {&t.entries, &t.pieces, &t.fixed, &t.slots,
                                        &t.funcs,   &t.cands,  &t.ukeys, &t.lin};
        std::vector<uint32_t>& v = *all[below(8)];
        switch (below(13)) {
            case 0: if (!v.empty()) v[below((uint32_t)v.size())] = rnd(); break;
            case 1: if (!v.empty()) v[below((uint32_t)v.size())] ^= 1u << below(32); break;
            case 2: if (!v.empty()) v.erase(v.begin() + below((uint32_t)v.size())); break;
            case 3: v.insert(v.begin() + below((uint32_t)v.size() + 1), rnd() & 0x1FFu); break;
            case 4: if (!v.empty()) v.pop_back(); break;
            case 5: if (t.n_resid) t.n_resid -= 1 + below(t.n_resid); break;
            case 6: if (t.gen.size() > 1) t.gen.pop_back();
                    else t.gen[0].width = 1 + below(8);
                    break;
            case 7: t.gen[below((uint32_t)t.gen.size())].width = 1 + below(256); break;
            case 8: if (t.n_roots) t.n_roots -= 1 + below(t.n_roots); break;
            case 9: if (t.n_atoms) t.n_atoms -= 1 + below(t.n_atoms); break;
            case 10: if (t.n_urows) t.n_urows -= 1 + below(t.n_urows); break;
            case 11: if (t.n_srows) t.n_srows -= 1 + below(t.n_srows); break;
            default: if (!v.empty()) v[below((uint32_t)v.size())] += 1 + below(2) * 255u;
        }
    }
}

static mg_uf_tables uf_of(const Tables& t) {
    // whole rows only: the counts are what the caller passes
    return {t.slots.data(), (uint32_t)t.slots.size() / 2, t.funcs.data(),
            (uint32_t)t.funcs.size() / 3, t.cands.data(), (uint32_t)t.cands.size() / 6,
            t.ukeys.data(), (uint32_t)t.ukeys.size() / 8, t.n_urows};
}

static bool accepted(const Tables& t) {
    const uint32_t n_entries = (uint32_t)t.entries.size() / 5;
    return mg_walk_sum_ok(t.entries.data(), n_entries, t.pieces.data(),
                          (uint32_t)t.pieces.size() / 4,
                          t.fixed.size() / 8 >= n_entries ? t.fixed.data() : nullptr,
                          t.lin.size() >= n_entries ? t.lin.data() : nullptr, t.n_srows,
                          t.gen.data(), (uint32_t)t.gen.size(), t.n_resid, t.n_roots, t.n_atoms,
                         uf_of(t));
}

static uint32_t* exact(const std::vector<uint32_t>& v, size_t words) {
    uint32_t* p = (uint32_t*)malloc(words * 4 + 1);
    if (words) memcpy(p, v.data(), words * 4);
    return p;
}

// every slot resolved and every lane of a few rounds on exactly-sized buffers;
// returns the lanes that applied an entry, *resolved: the slots with a leaf,
// *linear: the lanes that applied a linear entry
static uint32_t run(const Tables& t, uint32_t lanes, unsigned long long* resolved,
                    unsigned long long* linear) {
    const uint32_t n_leaves = (uint32_t)t.gen.size(), n_entries = (uint32_t)t.entries.size() / 5,
                   n_pieces = (uint32_t)t.pieces.size() / 4;
    const mg_uf_tables u = uf_of(t);
    const uint32_t n_rwords = MG_BOUND_MASK_WORDS(t.n_roots),
                   n_mwords = n_rwords + MG_BOUND_MASK_WORDS(t.n_atoms);
    // exact copies, so the vectors' spare capacity hides nothing
    uint32_t* entries = exact(t.entries, (size_t)n_entries * 5);
    uint32_t* fixed = exact(t.fixed, (size_t)n_entries * 8);
    uint32_t* lin = exact(t.lin, (size_t)n_entries);
    uint32_t* svals = (uint32_t*)malloc((size_t)t.n_srows * 32 + 1);
    for (uint32_t i = 0; i < t.n_srows * 8; ++i) svals[i] = rnd() ^ rnd() << 16;
    uint32_t* pieces = exact(t.pieces, (size_t)n_pieces * 4);
    uint32_t* slots = exact(t.slots, (size_t)u.n_slots * 2);
    uint32_t* funcs = exact(t.funcs, (size_t)u.n_funcs * 3);
    uint32_t* cands = exact(t.cands, (size_t)u.n_cands * 6);
    uint32_t* ukeys = exact(t.ukeys, (size_t)u.n_ukeys * 8);
    uint32_t* mvals = (uint32_t*)malloc((size_t)n_mwords * 4 + 1);
    uint32_t* inplace = (uint32_t*)malloc((size_t)n_leaves * 32);
    mg_leafgen* gen = (mg_leafgen*)malloc((size_t)n_leaves * sizeof(mg_leafgen));
    uint32_t* base = (uint32_t*)malloc((size_t)n_leaves * 32);
    uint32_t* dst = (uint32_t*)malloc((size_t)n_leaves * 32);
    uint32_t* rvals = (uint32_t*)malloc((size_t)t.n_resid * 32 + 1);
    uint32_t* urows = (uint32_t*)malloc((size_t)t.n_urows * 32 + 1);
    uint32_t* dest = (uint32_t*)malloc((size_t)u.n_slots * 4 + 1);
    uint32_t* live = (uint32_t*)malloc((size_t)(1 + n_entries) * 4);
    for (uint32_t i = 0; i < n_mwords; ++i) mvals[i] = rnd() ^ rnd() << 16;
    memcpy(gen, t.gen.data(), (size_t)n_leaves * sizeof(mg_leafgen));
    for (uint32_t i = 0; i < n_leaves; ++i) {
        // small values, so that keys meet arguments now and then
        for (uint32_t k = 0; k < 8; ++k) base[i * 8 + k] = below(3) ? (k ? 0u : below(4))
                                                                    : rnd() ^ rnd() << 16;
        mg_repair_mask(base + i * 8, gen[i].width);
    }
    for (uint32_t i = 0; i < t.n_urows * 8; ++i)
        urows[i] = below(3) ? (i % 8 ? 0u : below(4)) : rnd() ^ rnd() << 16;
    for (uint32_t i = 0; i < t.n_resid * 8; ++i) rvals[i] = below(3) ? rnd() ^ rnd() << 16 : 0u;
    for (uint32_t p = 0; p < t.n_resid; ++p)
        if (below(4) == 0) memset(rvals + p * 8, 0, 32);
    for (uint32_t s = 0; s < u.n_slots; ++s) {
        dest[s] = mg_walk_uf_resolve(slots, funcs, cands, ukeys, s, base, urows, 1);
        if (dest[s] != MG_AIM_NONE && dest[s] >= n_leaves) abort();
        *resolved += dest[s] != MG_AIM_NONE;
    }
    mg_walk_uf_live(entries, n_entries, pieces, below(8) ? rvals : nullptr, mvals, n_rwords, dest,
                    live);
    if (live[0] > n_entries) abort();
    uint32_t aimed = 0;
    for (uint32_t r = 0; r < 3; ++r)
        for (uint32_t j = 0; j < lanes; ++j) {
            memcpy(dst, base, (size_t)n_leaves * 32);
            mg_repair_moves mv;
            const uint32_t e = mg_walk_sum_lane(base, gen, nullptr, n_leaves, 0x1234567ull + r,
                                                r * 9973u, j, lanes, entries, pieces, fixed, lin,
                                                rvals, svals, live, dest, dst, 1, &mv);
            if (j % 3 == 0) {                     // on the base itself, as the adopt kernel
                memcpy(inplace, base, (size_t)n_leaves * 32);
                const uint32_t e2 = mg_walk_sum_lane(inplace, gen, nullptr, n_leaves,
                                                     0x1234567ull + r, r * 9973u, j, lanes,
                                                     entries, pieces, fixed, lin, rvals, svals,
                                                     live, dest, inplace, 1, nullptr);
                if (e2 != e || memcmp(inplace, dst, (size_t)n_leaves * 32)) {
                    fprintf(stderr, "lane %u in place differs\n", j);
                    abort();
                }
            }
            if (e != MG_AIM_NONE && (e >= n_entries || j == 0 || j > lanes / 4)) abort();
            aimed += e != MG_AIM_NONE;
            if (e != MG_AIM_NONE && lin[e]) ++*linear;
            for (uint32_t i = 0; i < n_leaves; ++i) {
                uint32_t v[8];
                memcpy(v, dst + i * 8, 32);
                mg_repair_mask(v, gen[i].width);
                if (memcmp(v, dst + i * 8, 32)) {
                    fprintf(stderr, "leaf %u beyond its width %u\n", i, gen[i].width);
                    abort();
                }
            }
            if (j == 0 && memcmp(dst, base, (size_t)n_leaves * 32)) abort();
        }
    free(entries); free(pieces); free(gen); free(base); free(dst); free(rvals); free(live);
    free(fixed); free(mvals); free(inplace); free(slots); free(funcs); free(cands); free(ukeys);
    free(urows); free(dest); free(lin); free(svals);
    return aimed;
}

int main(int argc, char** argv) {
    const long iterations = argc > 1 ? atol(argv[1]) : 2000;
    long valid_accepted = 0, mutated = 0, mutated_accepted = 0, random_accepted = 0;
    unsigned long long aimed = 0, resolved = 0, linear = 0;
    const uint32_t lane_counts[] = {1, 7, 8, 63, 64, 65, 256};
    for (long it = 0; it < iterations; ++it) {
        Tables t = valid();
        if (accepted(t)) {
            ++valid_accepted;
            aimed += run(t, lane_counts[below(7)], &resolved, &linear);
        }
        for (int m = 0; m < 4; ++m) {
            Tables u = t;
            mutate(u);
            ++mutated;
            if (accepted(u)) {
                ++mutated_accepted;
                run(u, lane_counts[below(6)], &resolved, &linear);
            }
        }
        Tables r;
        r.gen = t.gen;
        r.n_resid = below(4);
        r.n_roots = below(64);
        r.n_atoms = below(64);
        r.n_urows = below(16);
        r.n_srows = below(4);
        for (uint32_t i = 0, n = 5 * (1 + below(3)); i < n; ++i)
            r.entries.push_back(below(2) ? below(8) : rnd());
        r.fixed.assign(8 * (r.entries.size() / 5), 0u);
        for (size_t i = 0; i < r.entries.size() / 5; ++i)
            r.lin.push_back(below(2) ? below(4) | below(4) << MG_SUM_ROW_SHIFT : rnd());
        if (below(2)) r.fixed[below((uint32_t)r.fixed.size())] = rnd();
        for (uint32_t i = 0, n = 4 * below(6); i < n; ++i)
            r.pieces.push_back(below(2) ? below(64) : below(2) ? MG_UF_SLOT | below(4) : rnd());
        for (uint32_t i = 0, n = 2 * below(4); i < n; ++i) r.slots.push_back(below(2) ? below(4) : rnd());
        for (uint32_t i = 0, n = 3 * below(4); i < n; ++i) r.funcs.push_back(below(2) ? below(6) : rnd());
        for (uint32_t i = 0, n = 6 * below(8); i < n; ++i) r.cands.push_back(below(2) ? below(8) : rnd());
        for (uint32_t i = 0, n = 8 * below(3); i < n; ++i) r.ukeys.push_back(rnd());
        if (accepted(r)) {
            ++random_accepted;
            run(r, 16, &resolved, &linear);
        }
    }
    printf("{\"iterations\": %ld, \"valid_accepted\": %ld, \"mutated\": %ld, "
           "\"mutated_accepted\": %ld, \"random_accepted\": %ld, \"aimed_lanes\": %llu, "
           "\"resolved_slots\": %llu, \"linear_lanes\": %llu}\n",
           iterations, valid_accepted, mutated, mutated_accepted, random_accepted, aimed, resolved,
           linear);
    return 0;
}

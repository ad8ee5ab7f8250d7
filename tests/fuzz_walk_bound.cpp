// Sanitizer fuzz of the safety boundary of the aims for orders (DESIGN.md
// §3.13): csrc/mg_walk_bound.h alone.  Random valid tables (XOR and order
// entries), mutated copies and random words go through the validator
// (mg_walk_bound_ok); whatever it accepts is run through mg_walk_bound_live and
// mg_walk_bound_lane on buffers allocated at exactly the sizes the accepted
// counts imply, so a read or write outside the tables, the fixed values, the
// residual values, the mask state, the live list or the leaves is an ASan
// report, and a neighbour with a bit beyond a leaf's width aborts.  Every
// third run applies the lane to the base itself, as the adopt kernel does, and
// must give what a separate destination gives.  Stand-alone: its own main,
// built with g++ -fsanitize=address,undefined
// (tests/test_walk_bound_sanitize.py).
//
//   fuzz_walk_bound [iterations]   prints one JSON line of counters

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mg_walk_bound.h"

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
    std::vector<uint32_t> entries, pieces, fixed;
    uint32_t n_resid = 0, n_roots = 0, n_atoms = 0;
};

static Tables valid() {
    Tables t;
    const uint32_t widths[] = {1, 7, 8, 13, 31, 32, 33, 64, 100, 143, 160, 255, 256};
    const uint32_t n_leaves = 1 + below(below(4) ? 12 : 40);
    for (uint32_t i = 0; i < n_leaves; ++i) {
        mg_leafgen g;
        memset(&g, 0, sizeof g);
        g.width = below(3) ? widths[below(13)] : 1 + below(256);
        t.gen.push_back(g);
    }
    t.n_resid = 1 + below(12);
    t.n_roots = 1 + below(below(3) ? 40 : 1024);
    t.n_atoms = below(below(3) ? 70 : 1025);
    const uint32_t n_entries = below(8) == 0 ? MG_AIM_MAX_ENTRIES - below(2) : below(12);
    for (uint32_t e = 0; e < n_entries; ++e) {
        const uint32_t cnt = below(6) == 0 ? MG_AIM_MAX_PIECES : 1 + below(8);
        t.entries.push_back(below(t.n_resid));
        t.entries.push_back((uint32_t)t.pieces.size() / 4);
        t.entries.push_back(cnt);
        const uint32_t mode = below(5);
        t.entries.push_back(mode);
        t.entries.push_back(mode == MG_BOUND_XOR ? 0u :
                            t.n_atoms && below(2) ? MG_BOUND_ATOM | below(t.n_atoms)
                                                  : below(t.n_roots));
        for (uint32_t k = 0; k < 8; ++k)
            t.fixed.push_back(mode == MG_BOUND_XOR || below(3) == 0 ? 0u : rnd() ^ rnd() << 16);
        for (uint32_t q = 0; q < cnt; ++q) {
            const uint32_t leaf = below(n_leaves), w = t.gen[leaf].width;
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
        std::vector<uint32_t>& v = below(5) == 0 ? t.fixed : below(2) ? t.entries : t.pieces;
        switch (below(10)) {
            case 0: if (!v.empty()) v[below((uint32_t)v.size())] = rnd(); break;
            case 1: if (!v.empty()) v[below((uint32_t)v.size())] ^= 1u << below(32); break;
            case 2: if (!v.empty()) v.erase(v.begin() + below((uint32_t)v.size())); break;
            case 3: v.insert(v.begin() + below((uint32_t)v.size() + 1), rnd() & 0x1FFu); break;
            case 4: if (!v.empty()) v.pop_back(); break;
            case 5: if (t.n_resid) t.n_resid -= 1 + below(t.n_resid); break;
            case 6: if (t.gen.size() > 1) t.gen.pop_back();
                    else t.gen[0].width = 1 + below(8);
                    break;
            case 8: if (t.n_roots) t.n_roots -= 1 + below(t.n_roots); break;
            case 9: if (t.n_atoms) t.n_atoms -= 1 + below(t.n_atoms); break;
            default: if (!v.empty()) v[below((uint32_t)v.size())] += 1 + below(2) * 255u;
        }
    }
}

static bool accepted(const Tables& t) {
    // whole entries and pieces only: the counts are what the caller passes;
    // a fixed array shorter than the entries is the caller's null pointer
    const uint32_t n_entries = (uint32_t)t.entries.size() / 5;
    return mg_walk_bound_ok(t.entries.data(), n_entries, t.pieces.data(),
                            (uint32_t)t.pieces.size() / 4,
                            t.fixed.size() / 8 >= n_entries ? t.fixed.data() : nullptr,
                            t.gen.data(), (uint32_t)t.gen.size(), t.n_resid, t.n_roots, t.n_atoms);
}

// every lane of a few rounds on exactly-sized buffers; returns the lanes that
// applied an entry
static uint32_t run(const Tables& t, uint32_t lanes) {
    const uint32_t n_leaves = (uint32_t)t.gen.size(), n_entries = (uint32_t)t.entries.size() / 5,
                   n_pieces = (uint32_t)t.pieces.size() / 4;
    // exact copies, so the vectors' spare capacity hides nothing
    const uint32_t n_rwords = MG_BOUND_MASK_WORDS(t.n_roots),
                   n_mwords = n_rwords + MG_BOUND_MASK_WORDS(t.n_atoms);
    uint32_t* entries = (uint32_t*)malloc((size_t)n_entries * 20 + 1);
    uint32_t* fixed = (uint32_t*)malloc((size_t)n_entries * 32 + 1);
    uint32_t* mvals = (uint32_t*)malloc((size_t)n_mwords * 4 + 1);
    uint32_t* inplace = (uint32_t*)malloc((size_t)n_leaves * 32);
    uint32_t* pieces = (uint32_t*)malloc((size_t)n_pieces * 16 + 1);
    mg_leafgen* gen = (mg_leafgen*)malloc((size_t)n_leaves * sizeof(mg_leafgen));
    uint32_t* base = (uint32_t*)malloc((size_t)n_leaves * 32);
    uint32_t* dst = (uint32_t*)malloc((size_t)n_leaves * 32);
    uint32_t* rvals = (uint32_t*)malloc((size_t)t.n_resid * 32 + 1);
    uint32_t* live = (uint32_t*)malloc((size_t)(1 + n_entries) * 4);
    if (n_entries) memcpy(entries, t.entries.data(), (size_t)n_entries * 20);
    if (n_entries) memcpy(fixed, t.fixed.data(), (size_t)n_entries * 32);
    for (uint32_t i = 0; i < n_mwords; ++i) mvals[i] = rnd() ^ rnd() << 16;
    if (n_pieces) memcpy(pieces, t.pieces.data(), (size_t)n_pieces * 16);
    memcpy(gen, t.gen.data(), (size_t)n_leaves * sizeof(mg_leafgen));
    for (uint32_t i = 0; i < n_leaves; ++i) {
        for (uint32_t k = 0; k < 8; ++k) base[i * 8 + k] = rnd() ^ rnd() << 16;
        mg_repair_mask(base + i * 8, gen[i].width);
    }
    for (uint32_t i = 0; i < t.n_resid * 8; ++i) rvals[i] = below(3) ? rnd() ^ rnd() << 16 : 0u;
    for (uint32_t p = 0; p < t.n_resid; ++p)
        if (below(4) == 0) memset(rvals + p * 8, 0, 32);
    mg_walk_bound_live(entries, n_entries, below(8) ? rvals : nullptr, mvals, n_rwords, live);
    if (live[0] > n_entries) abort();
    uint32_t aimed = 0;
    for (uint32_t r = 0; r < 3; ++r)
        for (uint32_t j = 0; j < lanes; ++j) {
            memcpy(dst, base, (size_t)n_leaves * 32);
            mg_repair_moves mv;
            const uint32_t e = mg_walk_bound_lane(base, gen, nullptr, n_leaves, 0x1234567ull + r,
                                                  r * 9973u, j, lanes, entries, pieces, fixed,
                                                  rvals, live, dst, 1, &mv);
            if (j % 3 == 0) {                     // on the base itself, as the adopt kernel
                memcpy(inplace, base, (size_t)n_leaves * 32);
                const uint32_t e2 = mg_walk_bound_lane(inplace, gen, nullptr, n_leaves,
                                                       0x1234567ull + r, r * 9973u, j, lanes,
                                                       entries, pieces, fixed, rvals, live,
                                                       inplace, 1, nullptr);
                if (e2 != e || memcmp(inplace, dst, (size_t)n_leaves * 32)) {
                    fprintf(stderr, "lane %u in place differs\n", j);
                    abort();
                }
            }
            if (e != MG_AIM_NONE && (e >= n_entries || j == 0 || j > lanes / 4)) abort();
            aimed += e != MG_AIM_NONE;
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
    free(fixed); free(mvals); free(inplace);
    return aimed;
}

int main(int argc, char** argv) {
    const long iterations = argc > 1 ? atol(argv[1]) : 2000;
    long valid_accepted = 0, mutated = 0, mutated_accepted = 0, random_accepted = 0;
    unsigned long long aimed = 0;
    const uint32_t lane_counts[] = {1, 7, 8, 63, 64, 65, 256};
    for (long it = 0; it < iterations; ++it) {
        Tables t = valid();
        if (accepted(t)) {
            ++valid_accepted;
            aimed += run(t, lane_counts[below(7)]);
        }
        for (int m = 0; m < 4; ++m) {
            Tables u = t;
            mutate(u);
            ++mutated;
            if (accepted(u)) {
                ++mutated_accepted;
                run(u, lane_counts[below(6)]);
            }
        }
        Tables r;
        r.gen = t.gen;
        r.n_resid = below(4);
        r.n_roots = below(64);
        r.n_atoms = below(64);
        for (uint32_t i = 0, n = 5 * (1 + below(3)); i < n; ++i)
            r.entries.push_back(below(2) ? below(8) : rnd());
        r.fixed.assign(8 * (r.entries.size() / 5), 0u);
        if (below(2)) r.fixed[below((uint32_t)r.fixed.size())] = rnd();
        for (uint32_t i = 0, n = 4 * below(6); i < n; ++i)
            r.pieces.push_back(below(2) ? below(64) : rnd());
        if (accepted(r)) {
            ++random_accepted;
            run(r, 16);
        }
    }
    printf("{\"iterations\": %ld, \"valid_accepted\": %ld, \"mutated\": %ld, "
           "\"mutated_accepted\": %ld, \"random_accepted\": %ld, \"aimed_lanes\": %llu}\n",
           iterations, valid_accepted, mutated, mutated_accepted, random_accepted, aimed);
    return 0;
}

// Sanitizer fuzz of the tree scoring's safety boundary:
// csrc/mg_walk_tree.h alone.  Random valid tables, mutated copies and random
// words go through the validator (mg_walk_tree_ok); whatever it accepts is
// scored by mg_walk_tree_score_lane on buffers allocated at exactly the sizes
// the accepted counts imply, so a read outside the tables, the atom mask, the
// residual rows or the stack is an ASan report.  Stand-alone: its own main,
// built with g++ -fsanitize=address,undefined (tests/test_walk_tree_sanitize.py).
//
//   fuzz_walk_tree [iterations]   prints one JSON line of counters

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mg_walk_tree.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}
static uint32_t below(uint32_t n) { return n ? rnd() % n : 0; }

struct Tables {
    std::vector<uint32_t> roots, atoms, code;
    uint32_t n_resid = 0;
};

static uint32_t entry(uint32_t n_resid) {
    const uint32_t kind = n_resid ? below(MG_WALK_KINDS) : MG_WALK_FLAT;
    return kind << 16 | (kind == MG_WALK_FLAT ? 0u : below(n_resid));
}

// a random valid program: (words, atoms, stack) within the limits by construction
static void program(std::vector<uint32_t>& code, uint32_t n_atoms) {
    uint32_t depth = 0, n_atom_words = 0, words = 0;
    const uint32_t target = 1 + below(MG_WT_ROOT_WORDS - 2);
    while (words < target || depth != 1) {
        const bool must_pop = depth == MG_WT_STACK || words + depth >= MG_WT_ROOT_WORDS - 1;
        if (depth >= 1 && (must_pop || below(3) == 0)) {
            const uint32_t n = must_pop && depth > 1 ? 2 + below(depth - 1) : 1 + below(depth);
            code.push_back((below(2) ? MG_WT_AND : MG_WT_OR) << 16 | n);
            depth -= n - 1;
        } else if (n_atoms && n_atom_words < MG_WT_ROOT_ATOMS && below(8)) {
            code.push_back(MG_WT_ATOM << 16 | below(n_atoms));
            ++n_atom_words;
            ++depth;
        } else {
            code.push_back(MG_WT_PUSH_INF << 16);
            ++depth;
        }
        ++words;
        if (words >= MG_WT_ROOT_WORDS - 1 && depth == 1) break;
    }
    code.push_back(MG_WT_END << 16);
}

static Tables valid() {
    Tables t;
    const uint32_t sizes[] = {1, 2, 31, 32, 33, 64, 255, 256, 257, 1024};
    const uint32_t n_roots = below(4) ? 1 + below(40) : sizes[below(10)];
    const uint32_t n_atoms = below(4) ? below(40) : sizes[below(10)] - below(2);
    t.n_resid = below(3) ? 1 + below(12) : 0;
    for (uint32_t i = 0; i < n_atoms; ++i) t.atoms.push_back(entry(t.n_resid));
    for (uint32_t k = 0; k < n_roots; ++k) {
        if (below(3) == 0) {
            t.roots.push_back(entry(t.n_resid));
        } else {
            t.roots.push_back(MG_WT_TREE | (uint32_t)t.code.size());
            program(t.code, n_atoms);
        }
    }
    return t;
}

static void mutate(Tables& t) {
    const uint32_t n = 1 + below(3);
    for (uint32_t i = 0; i < n; ++i) {
        std::vector<uint32_t>& v = below(4) == 0 ? t.roots : below(3) == 0 ? t.atoms : t.code;
        switch (below(7)) {
            case 0: if (!v.empty()) v[below((uint32_t)v.size())] = rnd(); break;
            case 1: if (!v.empty()) v[below((uint32_t)v.size())] ^= 1u << below(32); break;
            case 2: if (!v.empty()) v.erase(v.begin() + below((uint32_t)v.size())); break;
            case 3: v.insert(v.begin() + below((uint32_t)v.size() + 1), rnd() & 0x7FFFFu); break;
            case 4: if (!v.empty()) v.pop_back(); break;
            case 5: if (t.n_resid) t.n_resid -= 1 + below(t.n_resid); break;
            default: if (!v.empty()) v[below((uint32_t)v.size())] += below(2) ? 1u : 0x10000u;
        }
    }
}

static bool accepted(const Tables& t) {
    return mg_walk_tree_ok(t.roots.data(), (uint32_t)t.roots.size(), t.atoms.data(),
                           (uint32_t)t.atoms.size(), t.code.data(), (uint32_t)t.code.size(),
                           t.n_resid);
}

// score `lanes` lanes on exactly-sized rows; returns the largest cost
static uint32_t score(const Tables& t, uint32_t lanes) {
    const uint32_t n_roots = (uint32_t)t.roots.size(), n_atoms = (uint32_t)t.atoms.size();
    // exact copies, so the vectors' spare capacity hides nothing
    std::vector<uint32_t> roots(t.roots), atoms(t.atoms), code(t.code);
    roots.shrink_to_fit();
    atoms.shrink_to_fit();
    code.shrink_to_fit();
    std::vector<uint32_t> masks((size_t)((n_roots + 255) / 256) * 8 * lanes);
    std::vector<uint32_t> amasks((size_t)((n_atoms + 255) / 256) * 8 * lanes);
    std::vector<uint32_t> resid((size_t)t.n_resid * 8 * lanes);
    for (auto& w : masks) w = below(4) ? rnd() | rnd() : rnd();
    for (auto& w : amasks) w = rnd();
    for (auto& w : resid) w = below(3) ? rnd() : 0u;
    uint32_t* stack = (uint32_t*)malloc(MG_WT_STACK * sizeof(uint32_t));
    uint32_t worst = 0;
    for (uint32_t a = 0; a < lanes; ++a) {
        uint32_t nfail = ~0u, cost = ~0u;
        mg_walk_tree_score_lane(masks.data(), amasks.empty() ? nullptr : amasks.data(),
                                resid.empty() ? nullptr : resid.data(), lanes, a, roots.data(),
                                atoms.empty() ? nullptr : atoms.data(),
                                code.empty() ? nullptr : code.data(), n_roots, true, stack, 1,
                                &nfail, &cost);
        if (nfail > n_roots || cost < nfail || cost > nfail * MG_WT_INF) {
            fprintf(stderr, "bad key: nfail %u cost %u of %u roots\n", nfail, cost, n_roots);
            abort();
        }
        worst = cost > worst ? cost : worst;
    }
    free(stack);
    return worst;
}

int main(int argc, char** argv) {
    const long iterations = argc > 1 ? atol(argv[1]) : 2000;
    long valid_accepted = 0, mutated = 0, mutated_accepted = 0, random_accepted = 0;
    uint32_t worst = 0;
    for (long it = 0; it < iterations; ++it) {
        Tables t = valid();
        if (accepted(t)) {
            ++valid_accepted;
            const uint32_t c = score(t, 1 + below(5));
            worst = c > worst ? c : worst;
        }
        for (int m = 0; m < 4; ++m) {
            Tables u = t;
            mutate(u);
            ++mutated;
            if (accepted(u)) {
                ++mutated_accepted;
                score(u, 1 + below(3));
            }
        }
        Tables r;
        r.n_resid = below(4);
        for (uint32_t i = 0, n = 1 + below(4); i < n; ++i)
            r.roots.push_back(below(2) ? MG_WT_TREE | below(24) : rnd());
        for (uint32_t i = 0, n = below(6); i < n; ++i) r.atoms.push_back(rnd());
        for (uint32_t i = 0, n = below(24); i < n; ++i) r.code.push_back(rnd());
        if (accepted(r)) {
            ++random_accepted;
            score(r, 2);
        }
    }
    printf("{\"iterations\": %ld, \"valid_accepted\": %ld, \"mutated\": %ld, "
           "\"mutated_accepted\": %ld, \"random_accepted\": %ld, \"worst_cost\": %u}\n",
           iterations, valid_accepted, mutated, mutated_accepted, random_accepted, worst);
    return 0;
}

// Sanitizer fuzz of the host side of mg_carry_census:
// csrc/mg_carry.h alone — the plan of its device buffer (mg_carry_census_plan)
// and the start rule in sequential form (mg_carry_pick_starts, with the
// per-entry predicate and the rank of a best that the starts kernel runs too).
// Random batches are planned and held to the ladder's plan on the regions they
// share; what fits a host allocation is laid out in a buffer of exactly the
// planned bytes, every region claimed at the size the ABI uses — a region that
// leaves the buffer is an ASan report, two that overlap abort.  In that buffer
// every job's counter blocks are written twice: once with random words (the
// rule must stay inside the blocks and the output block whatever they hold),
// once counted from random verdict bits, rung by rung over the rung's own
// columns.  On the counted blocks the starts are held to a list built from the
// bits directly, and the claim the rule rests on is checked: before the padding
// no column comes twice.  Walkers of 0 and 65, n_roots of 0 and 1025 and mask
// probes outside the program's are refused.  Stand-alone: its own main, built
// with g++ -fsanitize=address,undefined (tests/test_carry_census_sanitize.py).
//
//   fuzz_carry_census [iterations]   prints one JSON line of counters

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mg_carry.h"

static uint64_t g_state = 0x8CB92BA72F3D8DD7ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}
static uint32_t below(uint32_t n) { return n ? rnd() % n : 0; }

#define MAX_HOST_BYTES ((uint64_t)8 << 20)

struct batch {
    std::vector<uint32_t> leaves, rungs, roots, probes, probe0;
    uint32_t lanes = 1, walkers = 1, max_leaves = 0;
};

struct tally {
    unsigned long long laid = 0, bytes_laid = 0, jobs_picked = 0, random_picked = 0, padded = 0,
                       longer = 0, exact = 0, hits = 0, sole_starts = 0, distinct_checked = 0;
};

// The counter block of the columns col0 .. col0 + lanes - 1 from verdict bits
// (bits[c * roots + k]: root k holds on column c), as mg_census_block counts.
static void count_block(const std::vector<uint8_t>& bits, uint32_t roots, uint32_t col0,
                        uint32_t lanes, unsigned long long* out) {
    for (uint32_t k = 0; k < mg_census_words(roots); ++k)
        out[k] = k >= mg_census_sole_index(roots) ? ~0ull : 0ull;
    for (uint32_t c = col0; c < col0 + lanes; ++c) {
        uint32_t nfail = 0, first_fail = 0;
        for (uint32_t k = 0; k < roots; ++k) {
            if (bits[(uint64_t)c * roots + k]) {
                ++out[mg_census_pass(roots) + k];
            } else {
                if (!nfail) first_fail = k;
                ++nfail;
            }
        }
        ++out[mg_census_hist(roots) + nfail];
        if (nfail) ++out[mg_census_first(roots) + first_fail];
        if (nfail == 1) {
            ++out[mg_census_sole(roots) + first_fail];
            unsigned long long* si = out + mg_census_sole_index(roots) + first_fail;
            if (c < *si) *si = c;
        }
        const unsigned long long key = ((unsigned long long)nfail << MG_CENSUS_OFFSET_BITS) | c;
        if (key < out[mg_census_best(roots)]) out[mg_census_best(roots)] = key;
    }
}

// The list of the rule from the bits alone: per rung the column with the
// fewest failing roots (lowest first), those sorted by (failing, rung); then
// per rung and root the lowest column failing that root only, the rung's best
// left out.
static void list_from_bits(const std::vector<uint8_t>& bits, uint32_t roots, uint32_t rungs,
                           uint32_t lanes, std::vector<int64_t>* cols,
                           std::vector<uint32_t>* fails) {
    std::vector<uint32_t> nfail((size_t)rungs * lanes);
    for (uint32_t c = 0; c < rungs * lanes; ++c) {
        uint32_t f = 0;
        for (uint32_t k = 0; k < roots; ++k) f += !bits[(uint64_t)c * roots + k];
        nfail[c] = f;
    }
    std::vector<uint32_t> best(rungs);
    std::vector<uint32_t> order(rungs);
    for (uint32_t r = 0; r < rungs; ++r) {
        best[r] = r * lanes;
        for (uint32_t c = r * lanes; c < (r + 1) * lanes; ++c)
            if (nfail[c] < nfail[best[r]]) best[r] = c;
        order[r] = r;
    }
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return nfail[best[a]] < nfail[best[b]]; });
    for (uint32_t r : order) {
        cols->push_back(best[r]);
        fails->push_back(nfail[best[r]]);
    }
    for (uint32_t r = 0; r < rungs; ++r)
        for (uint32_t k = 0; k < roots; ++k)
            for (uint32_t c = r * lanes; c < (r + 1) * lanes; ++c)
                if (nfail[c] == 1 && !bits[(uint64_t)c * roots + k]) {
                    if (c != best[r]) {
                        cols->push_back(c);
                        fails->push_back(1);
                    }
                    break;
                }
}

// Lay the plan out in a buffer of exactly `bytes`, write counter blocks in
// their regions and pick the starts into the output block.
static void materialise(const batch& b, uint32_t cols, const std::vector<uint64_t>& off,
                        uint64_t bytes, uint64_t leaf_w, uint64_t probe_w, tally* t) {
    const uint32_t n = (uint32_t)b.leaves.size(), W = b.walkers;
    uint8_t* buf = (uint8_t*)malloc(bytes ? bytes : 1);
    uint8_t* seen = (uint8_t*)calloc(bytes ? bytes : 1, 1);
    if (!buf || !seen) abort();
    auto claim = [&](uint64_t at, uint64_t len) {
        if (at % 256) abort();                          // every region is aligned
        if (len && memchr(seen + at, 1, len)) abort();  // two regions overlap
        if (len) memset(seen + at, 1, len);
        if (len) memset(buf + at, 0, len);
        t->bytes_laid += len;
    };
    claim(off[MG_CY_DESCS], (uint64_t)n * sizeof(mg_pdesc));
    claim(off[MG_CY_JOBS], (uint64_t)n * sizeof(mg_carry_dev_job));
    claim(off[MG_CY_FIRST], (uint64_t)n * 8);
    claim(off[MG_CC_BASE(n) + MG_CC_RECORDS], (uint64_t)n * sizeof(mg_carry_census_dev_job));
    claim(off[MG_CY_OUT], (uint64_t)n * mg_carry_census_out_job(W, b.max_leaves));
    uint32_t most = 0, most_probes = 0;
    for (uint32_t g = 0; g < n; ++g) {
        const uint64_t k = b.leaves[g];
        most = b.leaves[g] > most ? b.leaves[g] : most;
        most_probes = b.probes[g] > most_probes ? b.probes[g] : most_probes;
        claim(off[MG_CY_OFF(g, MG_CY_MASK)], (k + 31) / 32 * 4 * b.rungs[g]);
        claim(off[MG_CY_OFF(g, MG_CY_ROWS)], k * 32);
        claim(off[MG_CY_OFF(g, MG_CY_GEN)], k * sizeof(mg_leafgen));
        claim(off[MG_CY_OFF(g, MG_CY_LEAVES)], k * 32 * cols);
        claim(off[MG_CC_OFF(n, g, MG_CC_COUNTS)],
              (uint64_t)mg_census_words(b.roots[g]) * b.rungs[g] * 8);
        claim(off[MG_CC_OFF(n, g, MG_CC_PROBES)], (uint64_t)b.probes[g] * 32 * cols);
    }
    // one download: the counters end where the output block begins; the probe
    // regions lie at a common stride and end the buffer
    uint64_t end = off[MG_CC_OFF(n, n - 1, MG_CC_COUNTS)] +
                   (uint64_t)mg_census_words(b.roots[n - 1]) * b.rungs[n - 1] * 8;
    end = (end + 255) & ~(uint64_t)255;
    if (end != off[MG_CY_OUT]) abort();
    if (probe_w * 4 < (uint64_t)most_probes * 32 * cols || probe_w * 4 % 256 ||
        probe_w * 4 >= (uint64_t)most_probes * 32 * cols + 256)
        abort();
    for (uint32_t g = 0; g < n; ++g) {
        if (off[MG_CY_OFF(g, MG_CY_LEAVES)] != off[MG_CY_OFF(0, MG_CY_LEAVES)] + g * leaf_w * 4)
            abort();
        if (off[MG_CC_OFF(n, g, MG_CC_PROBES)] != off[MG_CC_OFF(n, 0, MG_CC_PROBES)] + g * probe_w * 4)
            abort();
    }
    if (off[MG_CC_OFF(n, 0, MG_CC_PROBES)] != off[MG_CY_OFF(0, MG_CY_LEAVES)] + n * leaf_w * 4) abort();
    if (off[MG_CC_OFF(n, 0, MG_CC_PROBES)] + n * probe_w * 4 != bytes) abort();

    int64_t* out_col = (int64_t*)(buf + off[MG_CY_OUT]);
    uint32_t* out_nfail = (uint32_t*)(buf + off[MG_CY_OUT] + (uint64_t)n * W * 8);
    for (uint32_t g = 0; g < n; ++g) {
        const uint32_t roots = b.roots[g], rungs = b.rungs[g], lanes = b.lanes;
        unsigned long long* counts = (unsigned long long*)(buf + off[MG_CC_OFF(n, g, MG_CC_COUNTS)]);
        const uint64_t words = (uint64_t)mg_census_words(roots) * rungs;
        // any words at all: the rule reads the blocks and writes W entries
        for (uint64_t k = 0; k < words; ++k)
            counts[k] = below(3) ? ~0ull : ((uint64_t)rnd() << 32 | rnd());
        mg_carry_pick_starts(counts, roots, rungs, W, out_col + (uint64_t)g * W,
                             out_nfail + (uint64_t)g * W);
        ++t->random_picked;
        // counted from verdict bits; the styles make every situation common:
        // mostly true bits (hits and sole columns), one stubborn root, noise
        const uint32_t style = below(4);
        const uint32_t stubborn = below(roots), hit_rung = below(rungs);
        std::vector<uint8_t> bits((size_t)rungs * lanes * roots);
        for (uint32_t c = 0; c < rungs * lanes; ++c)
            for (uint32_t k = 0; k < roots; ++k) {
                uint8_t v = style == 3 ? below(2) : below(style == 0 ? 40 : 12) != 0;
                if (style == 1 && k == stubborn) v = 0;
                if (style == 2 && c / lanes != hit_rung && k == stubborn) v = 0;
                bits[(uint64_t)c * roots + k] = v;
            }
        for (uint32_t r = 0; r < rungs; ++r)
            count_block(bits, roots, r * lanes, lanes, counts + (uint64_t)r * mg_census_words(roots));
        int64_t* col = out_col + (uint64_t)g * W;
        uint32_t* nf = out_nfail + (uint64_t)g * W;
        mg_carry_pick_starts(counts, roots, rungs, W, col, nf);
        std::vector<int64_t> want_col;
        std::vector<uint32_t> want_nf;
        list_from_bits(bits, roots, rungs, lanes, &want_col, &want_nf);
        const size_t len = want_col.size();
        // no column twice before the padding
        std::vector<int64_t> sorted = want_col;
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) abort();
        t->distinct_checked += len;
        for (uint32_t w = 0; w < W; ++w) {
            const size_t src = w < len ? w : 0;
            if (col[w] != want_col[src] || nf[w] != want_nf[src]) abort();
            if (col[w] < 0 || col[w] >= (int64_t)rungs * lanes) abort();
            if (w < len && w >= rungs) ++t->sole_starts;
        }
        t->padded += len < W;
        t->longer += len > W;
        t->exact += len == W;
        t->hits += nf[0] == 0;
        ++t->jobs_picked;
    }
    free(buf);
    free(seen);
    ++t->laid;
}

static int plan(const batch& b, uint32_t n_jobs, std::vector<uint64_t>* off, uint64_t* bytes,
                uint64_t* leaf_w, uint64_t* probe_w) {
    off->assign(MG_CC_TABLE(b.leaves.size()), ~0ull);
    return mg_carry_census_plan(b.leaves.data(), b.rungs.data(), b.roots.data(), b.probes.data(),
                                b.probe0.data(), n_jobs, b.lanes, b.walkers, b.max_leaves,
                                off->data(), bytes, leaf_w, probe_w, nullptr);
}

// plan, compare with the ladder's plan, lay out what is small enough
static int drive(const batch& b, tally* t) {
    const uint32_t n = (uint32_t)b.leaves.size();
    std::vector<uint64_t> off;
    uint64_t bytes = 0, leaf_w = 0, probe_w = 0;
    const int st = plan(b, n, &off, &bytes, &leaf_w, &probe_w);
    if (st != MG_CC_OK) return st;
    std::vector<uint64_t> lad(MG_CY_SHARED + (size_t)n * MG_CY_JOB_REGIONS, ~0ull);
    uint64_t lad_bytes = 0, lad_leaf_w = 0;
    if (!mg_carry_ladder_plan(b.leaves.data(), b.rungs.data(), n, b.lanes, b.max_leaves, lad.data(),
                              &lad_bytes, &lad_leaf_w))
        abort();                                        // the census accepts no ladder refused
    // the uploaded front lies where the ladder has it, the leaf stride is the ladder's
    if (off[MG_CY_DESCS] != lad[MG_CY_DESCS] || off[MG_CY_JOBS] != lad[MG_CY_JOBS] ||
        off[MG_CY_FIRST] != lad[MG_CY_FIRST] || leaf_w != lad_leaf_w)
        abort();
    for (uint32_t g = 0; g < n; ++g)
        for (uint32_t k : {MG_CY_MASK, MG_CY_ROWS, MG_CY_GEN})
            if (off[MG_CY_OFF(g, k)] != lad[MG_CY_OFF(g, k)]) abort();
    if (off[MG_CC_BASE(n) + MG_CC_RECORDS] != lad[MG_CY_OUT]) abort();
    uint32_t cols = 0;
    if (!mg_carry_ladder_ok(b.rungs.data(), n, b.lanes, &cols)) abort();
    if (bytes % 256) abort();
    for (uint64_t o : off)
        if (o % 256 || o > bytes) abort();
    bool fits = true;
    for (uint32_t c : b.leaves) fits = fits && c <= b.max_leaves;
    if (fits && bytes <= MAX_HOST_BYTES) materialise(b, cols, off, bytes, leaf_w, probe_w, t);
    return MG_CC_OK;
}

int main(int argc, char** argv) {
    const long iterations = argc > 1 ? atol(argv[1]) : 1000;
    long valid_planned = 0, walkers_refused = 0, roots_refused = 0, mask_refused = 0,
         ladder_refused = 0, overflow_refused = 0;
    tally t;
    const uint32_t lane_counts[] = {1, 2, 7, 63, 64, 65, 256};
    const uint32_t root_counts[] = {1, 2, 3, 31, 32, 33, 256, 257, 1024};
    const uint32_t walker_counts[] = {1, 2, 4, 8, 64};
    for (long it = 0; it < iterations; ++it) {
        batch b;
        const uint32_t n = 1 + below(below(8) ? 3 : 12);
        b.lanes = lane_counts[below(it % 8 ? 5 : 7)];
        b.walkers = below(2) ? walker_counts[below(5)] : 1 + below(MG_CARRY_MAX_WALKERS);
        uint32_t most = 0;
        for (uint32_t g = 0; g < n; ++g) {
            b.leaves.push_back(below(6) ? below(6) : 30 + below(10));
            b.rungs.push_back(1 + below(MG_CARRY_MAX_RUNGS));
            b.roots.push_back(below(3) ? 1 + below(12) : below(8) ? root_counts[below(7)]
                                                                   : root_counts[below(9)]);
            const uint32_t n_mask = (b.roots[g] + 255) / 256;
            b.probe0.push_back(below(3));
            b.probes.push_back(b.probe0[g] + n_mask + below(3));
            most = b.leaves[g] > most ? b.leaves[g] : most;
        }
        b.max_leaves = most + below(3);
        if (drive(b, &t) != MG_CC_OK) abort();
        ++valid_planned;
        // walkers of 0 and 65 and beyond
        batch bad = b;
        bad.walkers = below(2) ? 0 : MG_CARRY_MAX_WALKERS + 1 + (below(2) ? 0 : rnd());
        if (drive(bad, &t) != MG_CC_WALKERS) abort();
        ++walkers_refused;
        // n_roots of 0 and 1025 and beyond, whichever job has them
        bad = b;
        bad.roots[below(n)] = below(2) ? 0 : MG_CENSUS_MAX_ROOTS + 1 + (below(2) ? 0 : rnd());
        if (drive(bad, &t) != MG_CC_ROOTS) abort();
        ++roots_refused;
        // mask probes that begin at or run past the program's probes
        bad = b;
        const uint32_t g = below(n);
        if (below(2))
            bad.probe0[g] = bad.probes[g] + below(3);
        else
            bad.probes[g] = bad.probe0[g] + (bad.roots[g] + 255) / 256 - 1;
        if (drive(bad, &t) != MG_CC_MASK) abort();
        ++mask_refused;
        // what the ladder refuses: n_rungs of 0 and 9, lanes of 0
        bad = b;
        if (below(2))
            bad.rungs[below(n)] = below(2) ? 0 : MG_CARRY_MAX_RUNGS + 1;
        else
            bad.lanes = 0;
        if (drive(bad, &t) != MG_CC_LADDER) abort();
        ++ladder_refused;
        // sizes beyond 64 bits: 256 jobs of 2^32 - 1 leaves at 2^20 columns
        if (it % 64 == 0) {
            batch big;
            big.leaves.assign(MG_CARRY_MAX_JOBS, 0xFFFFFFFFu);
            big.rungs.assign(MG_CARRY_MAX_JOBS, 8);
            big.roots.assign(MG_CARRY_MAX_JOBS, 1024);
            big.probes.assign(MG_CARRY_MAX_JOBS, 0xFFFFFFFFu);
            big.probe0.assign(MG_CARRY_MAX_JOBS, 0);
            big.lanes = 1u << 17;
            big.walkers = 64;
            big.max_leaves = 1;
            if (drive(big, &t) != MG_CC_OVERFLOW) abort();
            ++overflow_refused;
        }
    }
    printf("{\"iterations\": %ld, \"valid_planned\": %ld, \"walkers_refused\": %ld, "
           "\"roots_refused\": %ld, \"mask_refused\": %ld, \"ladder_refused\": %ld, "
           "\"overflow_refused\": %ld, \"laid_out\": %llu, \"bytes_laid\": %llu, "
           "\"jobs_picked\": %llu, \"random_picked\": %llu, \"padded\": %llu, \"longer\": %llu, "
           "\"exact\": %llu, \"hits\": %llu, \"sole_starts\": %llu, \"distinct_checked\": %llu}\n",
           iterations, valid_planned, walkers_refused, roots_refused, mask_refused, ladder_refused,
           overflow_refused, t.laid, t.bytes_laid, t.jobs_picked, t.random_picked, t.padded,
           t.longer, t.exact, t.hits, t.sole_starts, t.distinct_checked);
    return 0;
}

// Sanitizer fuzz of the host side of mg_carry_batch:
// csrc/mg_carry.h alone — the check of the shared counts
// (mg_carry_shared_ok), the check of a leaf table (mg_carry_gen_ok), the plan
// of the batch's device buffer (mg_carry_plan) and the fill kernel's lane
// function (mg_carry_fill_lane, with the generator mg_carry_gen).  Random
// valid batches, copies with one leaf count mutated and batches of random
// words go through the plan, with valid and out-of-range shared arguments.
// Whatever the plan accepts at a size a host can allocate is laid out in a
// buffer of exactly the planned bytes: the uploaded regions and the output
// block are claimed at the size the ABI writes, so a region that leaves the
// buffer is an ASan report and two regions that overlap abort; then every
// job's leaf region is written by the lane function itself under a random pin
// mask, from masks, rows and generator tables that lie in their own regions
// of that buffer.  Stand-alone: its own main, built with
// g++ -fsanitize=address,undefined (tests/test_carry_sanitize.py).
//
//   fuzz_carry [iterations]   prints one JSON line of counters

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mg_carry.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}
static uint32_t below(uint32_t n) { return n ? rnd() % n : 0; }

#define MAX_HOST_BYTES ((uint64_t)8 << 20)
#define N_CONSTS 6u

static uint32_t g_consts[N_CONSTS * 8];

static mg_leafgen valid_gen() {
    static const uint32_t widths[] = {1, 8, 31, 32, 33, 64, 160, 255, 256};
    mg_leafgen g;
    g.width = below(2) ? widths[below(9)] : 1 + below(256);
    g.pool_n = below(3) ? below(N_CONSTS + 1) : 0;
    g.pool_off = g.pool_n ? below(N_CONSTS - g.pool_n + 1) : below(4);
    const bool search = below(2);
    g.pct_uniform = search ? 20 : 50;
    g.pct_small = search ? 40 : 70;
    g.pct_boundary = search ? 60 : 85;
    return g;
}

struct tally {
    unsigned long long laid = 0, bytes_laid = 0, lanes_filled = 0, pinned = 0, generated = 0,
                       classes[4] = {0, 0, 0, 0};
};

// Lay the plan out in a buffer of exactly `bytes` and fill every leaf region.
static void materialise(const std::vector<uint32_t>& counts, uint32_t lanes, uint32_t max_leaves,
                        const std::vector<uint64_t>& off, uint64_t bytes, uint64_t leaf_w,
                        tally* t) {
    const uint32_t n = (uint32_t)counts.size();
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
    claim(off[MG_CY_OUT], (uint64_t)n * 8 + (uint64_t)n * max_leaves * 32);
    uint32_t most = 0;
    for (uint32_t g = 0; g < n; ++g) {
        const uint64_t k = counts[g];
        most = counts[g] > most ? counts[g] : most;
        claim(off[MG_CY_OFF(g, MG_CY_MASK)], (k + 31) / 32 * 4);
        claim(off[MG_CY_OFF(g, MG_CY_ROWS)], k * 32);
        claim(off[MG_CY_OFF(g, MG_CY_GEN)], k * sizeof(mg_leafgen));
        claim(off[MG_CY_OFF(g, MG_CY_LEAVES)], k * 32 * lanes);
    }
    // the stride is the batch's maximum, and job g's region lies g strides on
    if (leaf_w * 4 < (uint64_t)most * 32 * lanes || leaf_w * 4 % 256 ||
        leaf_w * 4 >= (uint64_t)most * 32 * lanes + 256)
        abort();
    for (uint32_t g = 0; g < n; ++g)
        if (off[MG_CY_OFF(g, MG_CY_LEAVES)] != off[MG_CY_OFF(0, MG_CY_LEAVES)] + g * leaf_w * 4)
            abort();
    if (off[MG_CY_OFF(0, MG_CY_LEAVES)] + n * leaf_w * 4 != bytes) abort();
    // the fill: tables in their regions, the lane function into the leaf region
    const uint64_t seed = (uint64_t)rnd() << 32 | rnd(), prog_seed = rnd();
    const uint64_t first = below(2) ? ((uint64_t)1 << 32) + rnd() : rnd() % 200;
    for (uint32_t g = 0; g < n; ++g) {
        const uint32_t k = counts[g];
        uint32_t* mask = (uint32_t*)(buf + off[MG_CY_OFF(g, MG_CY_MASK)]);
        uint32_t* rows = (uint32_t*)(buf + off[MG_CY_OFF(g, MG_CY_ROWS)]);
        mg_leafgen* gen = (mg_leafgen*)(buf + off[MG_CY_OFF(g, MG_CY_GEN)]);
        uint32_t* leaves = (uint32_t*)(buf + off[MG_CY_OFF(g, MG_CY_LEAVES)]);
        const uint32_t style = below(4);                // none, all, random, random
        for (uint32_t w = 0; w < (k + 31) / 32; ++w)
            mask[w] = style == 0 ? 0u : style == 1 ? 0xFFFFFFFFu : rnd() ^ rnd() << 16;
        for (uint32_t l = 0; l < k; ++l) {
            gen[l] = valid_gen();
            for (uint32_t j = 0; j < 8; ++j) rows[(uint64_t)l * 8 + j] = rnd() ^ rnd() << 16;
        }
        if (!mg_carry_gen_ok(gen, k, N_CONSTS)) abort();
        for (uint32_t l = 0; l < k; ++l)
            for (uint32_t i = 0; i < lanes; ++i) {
                mg_carry_fill_lane(mask, rows, gen, g_consts, prog_seed, seed, first, l, i, lanes,
                                   i, leaves);
                // masked to the width, upper limbs zero; a pinned leaf is its row
                uint32_t v[8], want[8];
                for (uint32_t j = 0; j < 8; ++j) {
                    v[j] = leaves[((uint64_t)l * 8 + j) * lanes + i];
                    want[j] = v[j];
                }
                mg_repair_mask(want, gen[l].width);
                if (memcmp(v, want, 32)) abort();
                if (mg_carry_pinned(mask, l)) {
                    for (uint32_t j = 0; j < 8; ++j) want[j] = rows[(uint64_t)l * 8 + j];
                    mg_repair_mask(want, gen[l].width);
                    if (memcmp(v, want, 32)) abort();
                    ++t->pinned;
                } else {
                    const uint32_t br = mg_carry_branch(
                        gen[l], mg_carry_class(seed, prog_seed, l, first + i));
                    if (br > 3) abort();
                    ++t->classes[br];
                    ++t->generated;
                }
            }
        t->lanes_filled += (uint64_t)k * lanes;
    }
    free(buf);
    free(seen);
    ++t->laid;
}

// plan and lay out what is accepted and small enough; true when accepted
static bool drive(const std::vector<uint32_t>& counts, uint32_t n_jobs, uint32_t lanes,
                  uint32_t max_leaves, tally* t) {
    std::vector<uint64_t> off(MG_CY_SHARED + counts.size() * MG_CY_JOB_REGIONS, ~0ull);
    uint64_t bytes = 0, leaf_w = 0;
    if (!mg_carry_plan(counts.data(), n_jobs, lanes, max_leaves, off.data(), &bytes, &leaf_w))
        return false;
    if (n_jobs != counts.size() || bytes % 256) abort();
    for (uint64_t o : off)
        if (o % 256 || o > bytes) abort();
    bool fits = true;
    for (uint32_t c : counts) fits = fits && c <= max_leaves;
    if (fits && bytes <= MAX_HOST_BYTES) materialise(counts, lanes, max_leaves, off, bytes, leaf_w, t);
    return true;
}

int main(int argc, char** argv) {
    const long iterations = argc > 1 ? atol(argv[1]) : 2000;
    for (uint32_t i = 0; i < N_CONSTS * 8; ++i) g_consts[i] = i < 8 ? 0xFFFFFFFFu : rnd();
    long valid_planned = 0, mutated = 0, mutated_planned = 0, random_planned = 0,
         shared_refused = 0, gen_refused = 0, overflow_refused = 0;
    tally t;
    const uint32_t lane_counts[] = {1, 2, 63, 64, 65, 255, 256, 257};
    for (long it = 0; it < iterations; ++it) {
        const uint32_t n = 1 + below(below(8) ? 5 : 40);
        const uint32_t lanes = lane_counts[below(8)];
        std::vector<uint32_t> counts(n);
        uint32_t most = 0;
        for (uint32_t& c : counts) {
            c = below(6) ? below(12) : 30 + below(40);       // some past one mask word, some 0
            most = c > most ? c : most;
        }
        const uint32_t max_leaves = most + below(3);
        valid_planned += drive(counts, n, lanes, max_leaves, &t);
        for (int m = 0; m < 2; ++m) {
            std::vector<uint32_t> u = counts;
            uint32_t& c = u[below(n)];
            switch (below(4)) {
            case 0: c = 0; break;
            case 1: c += 1 + below(64); break;
            case 2: c = 0xFFFFFFFFu - below(3); break;
            default: c = rnd(); break;
            }
            ++mutated;
            // the plan does not depend on max_leaves covering the counts
            mutated_planned += drive(u, n, lanes, max_leaves, &t);
        }
        std::vector<uint32_t> r(n);
        for (uint32_t& c : r) c = below(3) ? rnd() : below(300);
        random_planned += drive(r, n, below(2) ? lanes : 1 + below(MG_REPAIR_MAX_LANES), rnd(), &t);
        // sizes beyond 64 bits are refused: 256 jobs of 2^32 - 1 leaves at 2^20 lanes
        if (it % 64 == 0) {
            std::vector<uint32_t> big(MG_CARRY_MAX_JOBS, 0xFFFFFFFFu);
            if (drive(big, MG_CARRY_MAX_JOBS, MG_REPAIR_MAX_LANES, 1, &t)) abort();
            ++overflow_refused;
        }
        // shared arguments out of range are refused whatever the counts
        const uint32_t bad = below(5);
        const uint32_t bn = bad == 0 ? 0 : bad == 1 ? MG_CARRY_MAX_JOBS + 1 + below(1000) : n;
        const uint32_t bl = bad == 2 ? 0 : bad == 3 ? MG_REPAIR_MAX_LANES + 1 + below(1000) : lanes;
        const bool ok = drive(counts, bn, bl, max_leaves, &t);
        if (ok != (bad == 4) || mg_carry_shared_ok(bn, bl) != (bad == 4)) abort();
        shared_refused += !ok;
        // a leaf table outside the constants or with a bad width is refused
        mg_leafgen g = valid_gen();
        if (!mg_carry_gen_ok(&g, 1, N_CONSTS)) abort();
        switch (below(4)) {
        case 0: g.width = 0; break;
        case 1: g.width = 257 + below(1000); break;
        case 2: g.pool_n = 1 + below(3); g.pool_off = N_CONSTS - g.pool_n + 1 + below(3); break;
        default: g.pool_n = 1 + below(3); g.pool_off = 0xFFFFFFFFu - below(2); break;
        }
        if (mg_carry_gen_ok(&g, 1, N_CONSTS)) abort();
        ++gen_refused;
    }
    printf("{\"iterations\": %ld, \"valid_planned\": %ld, \"mutated\": %ld, "
           "\"mutated_planned\": %ld, \"random_planned\": %ld, \"shared_refused\": %ld, "
           "\"gen_refused\": %ld, \"overflow_refused\": %ld, \"laid_out\": %llu, "
           "\"bytes_laid\": %llu, \"lanes_filled\": %llu, \"pinned\": %llu, \"generated\": %llu, "
           "\"classes\": [%llu, %llu, %llu, %llu]}\n",
           iterations, valid_planned, mutated, mutated_planned, random_planned, shared_refused,
           gen_refused, overflow_refused, t.laid, t.bytes_laid, t.lanes_filled, t.pinned,
           t.generated, t.classes[0], t.classes[1], t.classes[2], t.classes[3]);
    return 0;
}

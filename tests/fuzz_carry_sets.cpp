// Sanitizer fuzz of the host side of mg_carry_ladder_sets:
// csrc/mg_carry.h alone — the check of the shared counts (mg_carry_sets_ok),
// the check of a job's rung_set (mg_carry_rung_set_ok), the plan of the device
// buffer (mg_carry_sets_plan) and the set fill kernel's lane function
// (mg_carry_fill_set_lane).  Random batches with a random n_rungs (1..8) and
// n_sets (1..8) per job at lanes of 1, 63, 64, 65 and 256 are planned; what
// fits a host allocation is laid out in a buffer of exactly the planned bytes,
// every region claimed at the size the ABI writes — a region that leaves the
// buffer is an ASan report, two that overlap abort — and every job's leaf
// region of R x lanes columns is written by the lane function from masks, row
// sets, rung_set and generator tables that lie in their own regions of that
// buffer.  Every column is then held to mg_carry_fill_lane under the mask of
// its rung and the rows of that rung's set at candidate col % lanes, the
// surplus columns of a job with fewer rungs than the batch to its last rung.
// n_sets of 0 and 9, a rung_set entry out of range, R x lanes above 2^20 and
// sizes beyond 64 bits are refused.  Stand-alone: its own main, built with
// g++ -fsanitize=address,undefined (tests/test_carry_sets_sanitize.py).
//
//   fuzz_carry_sets [iterations]   prints one JSON line of counters

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
    unsigned long long laid = 0, bytes_laid = 0, cols_filled = 0, pinned = 0, generated = 0,
                       surplus = 0, set_cols[MG_CARRY_MAX_SETS] = {0};
};

// Lay the plan out in a buffer of exactly `bytes` and fill every leaf region.
static void materialise(const std::vector<uint32_t>& counts, const std::vector<uint32_t>& rungs,
                        const std::vector<uint32_t>& sets, uint32_t lanes, uint32_t cols,
                        uint32_t max_leaves, const std::vector<uint64_t>& off, uint64_t bytes,
                        uint64_t leaf_w, tally* t) {
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
    claim(off[MG_CS_BASE(n) + MG_CS_RECORDS], (uint64_t)n * sizeof(mg_carry_sets_dev_job));
    claim(off[MG_CY_OUT], (uint64_t)n * 16 + (uint64_t)n * max_leaves * 32);
    uint32_t most = 0;
    for (uint32_t g = 0; g < n; ++g) {
        const uint64_t k = counts[g];
        most = counts[g] > most ? counts[g] : most;
        claim(off[MG_CY_OFF(g, MG_CY_MASK)], (k + 31) / 32 * 4 * rungs[g]);
        claim(off[MG_CY_OFF(g, MG_CY_ROWS)], k * 32 * sets[g]);
        claim(off[MG_CY_OFF(g, MG_CY_GEN)], k * sizeof(mg_leafgen));
        claim(off[MG_CS_OFF(n, g, MG_CS_RUNG_SET)], (uint64_t)rungs[g] * 4);
        claim(off[MG_CY_OFF(g, MG_CY_LEAVES)], k * 32 * cols);
    }
    // everything uploaded lies before the output block, the leaf regions after it
    if (off[MG_CS_BASE(n) + MG_CS_RECORDS] >= off[MG_CY_OUT]) abort();
    for (uint32_t g = 0; g < n; ++g)
        if (off[MG_CS_OFF(n, g, MG_CS_RUNG_SET)] >= off[MG_CY_OUT] ||
            off[MG_CY_OFF(g, MG_CY_GEN)] > off[MG_CS_BASE(n) + MG_CS_RECORDS])
            abort();                                    // (a job of no leaves: empty regions)
    // the stride is the batch's maximum, and job g's region lies g strides on
    if (leaf_w * 4 < (uint64_t)most * 32 * cols || leaf_w * 4 % 256 ||
        leaf_w * 4 >= (uint64_t)most * 32 * cols + 256)
        abort();
    for (uint32_t g = 0; g < n; ++g)
        if (off[MG_CY_OFF(g, MG_CY_LEAVES)] != off[MG_CY_OFF(0, MG_CY_LEAVES)] + g * leaf_w * 4)
            abort();
    if (off[MG_CY_OFF(0, MG_CY_LEAVES)] + n * leaf_w * 4 != bytes) abort();
    const uint64_t seed = (uint64_t)rnd() << 32 | rnd(), prog_seed = rnd();
    const uint64_t first = below(2) ? ((uint64_t)1 << 32) + rnd() : rnd() % 200;
    for (uint32_t g = 0; g < n; ++g) {
        const uint32_t k = counts[g], words = (k + 31) / 32;
        uint32_t* masks = (uint32_t*)(buf + off[MG_CY_OFF(g, MG_CY_MASK)]);
        uint32_t* rows = (uint32_t*)(buf + off[MG_CY_OFF(g, MG_CY_ROWS)]);
        mg_leafgen* gen = (mg_leafgen*)(buf + off[MG_CY_OFF(g, MG_CY_GEN)]);
        uint32_t* rung_set = (uint32_t*)(buf + off[MG_CS_OFF(n, g, MG_CS_RUNG_SET)]);
        uint32_t* leaves = (uint32_t*)(buf + off[MG_CY_OFF(g, MG_CY_LEAVES)]);
        for (uint32_t w = 0; w < words * rungs[g]; ++w) {
            const uint32_t style = below(4);            // none, all, random, random
            masks[w] = style == 0 ? 0u : style == 1 ? 0xFFFFFFFFu : rnd() ^ rnd() << 16;
        }
        for (uint32_t r = 0; r < rungs[g]; ++r) rung_set[r] = below(sets[g]);
        rung_set[below(rungs[g])] = sets[g] - 1;        // the last row set is read
        if (!mg_carry_rung_set_ok(rung_set, rungs[g], sets[g])) abort();
        for (uint32_t l = 0; l < k; ++l) gen[l] = valid_gen();
        for (uint64_t i = 0; i < (uint64_t)k * 8 * sets[g]; ++i) rows[i] = rnd() ^ rnd() << 16;
        if (!mg_carry_gen_ok(gen, k, N_CONSTS)) abort();
        for (uint32_t l = 0; l < k; ++l)
            for (uint32_t c = 0; c < cols; ++c)
                mg_carry_fill_set_lane(masks, words, rungs[g], rung_set, rows, k, gen, g_consts,
                                       prog_seed, seed, first, l, c, lanes, cols, c, leaves);
        // rung by rung: the one-mask lane function under the rung's mask and
        // the rows of the rung's set, at `lanes` columns
        std::vector<uint32_t> want((size_t)k * 8 * lanes + 1);
        for (uint32_t r = 0; r < cols / lanes; ++r) {
            const uint32_t rr = r < rungs[g] ? r : rungs[g] - 1;
            const uint32_t* mask = masks + (uint64_t)rr * words;
            const uint32_t* set = rows + (uint64_t)rung_set[rr] * k * 8;
            for (uint32_t l = 0; l < k; ++l)
                for (uint32_t i = 0; i < lanes; ++i) {
                    mg_carry_fill_lane(mask, set, gen, g_consts, prog_seed, seed, first, l, i,
                                       lanes, i, want.data());
                    // a pinned leaf holds the row of the rung's set, masked to its width
                    uint32_t v[8];
                    const bool pin = mg_carry_pinned(mask, l);
                    if (pin) {
                        for (uint32_t j = 0; j < 8; ++j) v[j] = set[(uint64_t)l * 8 + j];
                        mg_repair_mask(v, gen[l].width);
                        ++t->pinned;
                    } else {
                        ++t->generated;
                    }
                    for (uint32_t j = 0; j < 8; ++j) {
                        const uint32_t got =
                            leaves[((uint64_t)l * 8 + j) * cols + (uint64_t)r * lanes + i];
                        if (got != want[((uint64_t)l * 8 + j) * lanes + i]) abort();
                        if (pin && got != v[j]) abort();
                    }
                }
            t->set_cols[rung_set[rr]] += (uint64_t)k * lanes;
            if (r >= rungs[g]) t->surplus += (uint64_t)k * lanes;
        }
        t->cols_filled += (uint64_t)k * cols;
    }
    free(buf);
    free(seen);
    ++t->laid;
}

// plan and lay out what is accepted and small enough; true when accepted
static bool drive(const std::vector<uint32_t>& counts, const std::vector<uint32_t>& rungs,
                  const std::vector<uint32_t>& sets, uint32_t n_jobs, uint32_t lanes,
                  uint32_t max_leaves, tally* t) {
    std::vector<uint64_t> off(MG_CS_TABLE(counts.size()), ~0ull);
    uint64_t bytes = 0, leaf_w = 0;
    uint32_t cols = 0;
    const bool ok = mg_carry_sets_ok(rungs.data(), sets.data(), n_jobs, lanes, &cols);
    if (!mg_carry_sets_plan(counts.data(), rungs.data(), sets.data(), n_jobs, lanes, max_leaves,
                            off.data(), &bytes, &leaf_w))
        return false;
    if (!ok) abort();                                   // the plan accepts no counts the check refuses
    uint32_t top = 0;
    for (uint32_t r : rungs) top = r > top ? r : top;
    if (n_jobs != counts.size() || bytes % 256 || cols != top * lanes || cols > (1u << 20)) abort();
    for (uint64_t o : off)
        if (o % 256 || o > bytes) abort();
    // with one set each the uploaded front lies at the ladder's own offsets
    bool fits = true, single = true;
    for (uint32_t c : counts) fits = fits && c <= max_leaves;
    for (uint32_t s : sets) single = single && s == 1;
    if (single) {
        std::vector<uint64_t> lad(MG_CY_SHARED + counts.size() * MG_CY_JOB_REGIONS, ~0ull);
        uint64_t lb = 0, lw = 0;
        if (!mg_carry_ladder_plan(counts.data(), rungs.data(), n_jobs, lanes, max_leaves,
                                  lad.data(), &lb, &lw) || lw != leaf_w)
            abort();
        for (uint32_t g = 0; g < n_jobs; ++g)
            for (uint32_t k = 0; k < MG_CY_LEAVES; ++k)
                if (lad[MG_CY_OFF(g, k)] != off[MG_CY_OFF(g, k)]) abort();
    }
    if (fits && bytes <= MAX_HOST_BYTES)
        materialise(counts, rungs, sets, lanes, cols, max_leaves, off, bytes, leaf_w, t);
    return true;
}

int main(int argc, char** argv) {
    const long iterations = argc > 1 ? atol(argv[1]) : 1000;
    for (uint32_t i = 0; i < N_CONSTS * 8; ++i) g_consts[i] = i < 8 ? 0xFFFFFFFFu : rnd();
    long valid_planned = 0, sets_refused = 0, rung_set_refused = 0, cols_refused = 0,
         shared_refused = 0, overflow_refused = 0;
    tally t;
    const uint32_t lane_counts[] = {1, 63, 64, 65, 256};
    for (long it = 0; it < iterations; ++it) {
        const uint32_t n = 1 + below(below(8) ? 4 : 24);
        const uint32_t lanes = lane_counts[below(5)];
        std::vector<uint32_t> counts(n), rungs(n), sets(n);
        uint32_t most = 0;
        for (uint32_t g = 0; g < n; ++g) {
            counts[g] = below(6) ? below(10) : 30 + below(40);   // some past one mask word, some 0
            rungs[g] = 1 + below(MG_CARRY_MAX_RUNGS);
            sets[g] = below(4) ? 1 + below(MG_CARRY_MAX_SETS) : 1;
            most = counts[g] > most ? counts[g] : most;
        }
        const uint32_t max_leaves = most + below(3);
        valid_planned += drive(counts, rungs, sets, n, lanes, max_leaves, &t);
        // n_sets of 0 and 9 (and beyond) are refused, whichever job has them
        std::vector<uint32_t> bad = sets;
        bad[below(n)] = below(2) ? 0 : MG_CARRY_MAX_SETS + 1 + (below(2) ? 0 : rnd());
        if (drive(counts, rungs, bad, n, lanes, max_leaves, &t)) abort();
        std::vector<uint64_t> unused(MG_CS_TABLE(n));
        uint64_t unused_bytes = 0;
        if (mg_carry_sets_plan(counts.data(), rungs.data(), nullptr, n, lanes, max_leaves,
                               unused.data(), &unused_bytes, nullptr))
            abort();                                    // and a null n_sets
        ++sets_refused;
        // a rung_set entry at or above n_sets, and a null rung_set
        {
            const uint32_t r = 1 + below(MG_CARRY_MAX_RUNGS), s = 1 + below(MG_CARRY_MAX_SETS);
            std::vector<uint32_t> rs(r);
            for (uint32_t& x : rs) x = below(s);
            if (!mg_carry_rung_set_ok(rs.data(), r, s)) abort();
            rs[below(r)] = s + (below(2) ? 0 : rnd() % 1000);
            if (mg_carry_rung_set_ok(rs.data(), r, s) || mg_carry_rung_set_ok(nullptr, r, s))
                abort();
            ++rung_set_refused;
        }
        // R x lanes above 2^20: refused; at 2^20 exactly: accepted
        std::vector<uint32_t> one(n, 1);
        const uint32_t top = 2 + below(MG_CARRY_MAX_RUNGS - 1);
        one[below(n)] = top;
        const uint32_t fit = (1u << 20) / top;
        std::vector<uint32_t> none(n, 0);
        if (drive(none, one, sets, n, fit + 1 + below(1000), 0, &t)) abort();
        if (!drive(none, one, sets, n, fit, 0, &t)) abort();
        ++cols_refused;
        // the shared counts of mg_carry_batch and the ladder's n_rungs hold here too
        const uint32_t kind = below(5);
        const uint32_t bn = kind == 0 ? 0 : kind == 1 ? MG_CARRY_MAX_JOBS + 1 + below(1000) : n;
        const uint32_t bl = kind == 2 ? 0 : kind == 3 ? MG_REPAIR_MAX_LANES + 1 + below(1000) : lanes;
        const uint32_t m2 = bn > n ? bn : n;
        std::vector<uint32_t> c2(m2, 1), r2(m2, 1), s2(m2, 1);
        if (kind == 4) r2[below(n)] = below(2) ? 0 : MG_CARRY_MAX_RUNGS + 1;
        if (drive(c2, r2, s2, bn, bl, 1, &t)) abort();
        ++shared_refused;
        // sizes beyond 64 bits: 256 jobs of 8 sets of 2^32 - 1 leaves at 2^20 columns
        if (it % 64 == 0) {
            std::vector<uint32_t> big(MG_CARRY_MAX_JOBS, 0xFFFFFFFFu), r8(MG_CARRY_MAX_JOBS, 8),
                s8(MG_CARRY_MAX_JOBS, MG_CARRY_MAX_SETS);
            if (drive(big, r8, s8, MG_CARRY_MAX_JOBS, 1u << 17, 1, &t)) abort();
            ++overflow_refused;
        }
    }
    printf("{\"iterations\": %ld, \"valid_planned\": %ld, \"sets_refused\": %ld, "
           "\"rung_set_refused\": %ld, \"cols_refused\": %ld, \"shared_refused\": %ld, "
           "\"overflow_refused\": %ld, \"laid_out\": %llu, \"bytes_laid\": %llu, "
           "\"cols_filled\": %llu, \"pinned\": %llu, \"generated\": %llu, \"surplus\": %llu, "
           "\"set_cols\": [",
           iterations, valid_planned, sets_refused, rung_set_refused, cols_refused, shared_refused,
           overflow_refused, t.laid, t.bytes_laid, t.cols_filled, t.pinned, t.generated, t.surplus);
    for (uint32_t s = 0; s < MG_CARRY_MAX_SETS; ++s)
        printf("%s%llu", s ? ", " : "", t.set_cols[s]);
    printf("]}\n");
    return 0;
}

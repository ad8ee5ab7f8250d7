// Sanitizer fuzz of the host side of mg_walk_batch:
// csrc/mg_walk_batch.h alone, the check of a job's counts
// (mg_walk_batch_shape_ok) and the plan of the batch's device buffer
// (mg_walk_batch_plan).  Random valid shapes, copies with one count mutated
// and shapes of random words go through both, with valid and random shared
// arguments.  Whatever the plan accepts at a size a host can allocate is laid
// out in a buffer of exactly the planned bytes: every region is written at the
// size the ABI uploads, clears or lets the kernels write (what the counts
// imply), so a region that leaves the buffer is an ASan report, and a byte
// written twice — two regions that overlap — aborts.  Stand-alone: its own
// main, built with g++ -fsanitize=address,undefined
// (tests/test_walk_batch_sanitize.py).
//
//   fuzz_walk_batch [iterations]   prints one JSON line of counters

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mg_walk_batch.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}
static uint32_t below(uint32_t n) { return n ? rnd() % n : 0; }

static mg_walk_shape valid() {
    mg_walk_shape s;
    s.n_leaves = 1 + below(12);
    s.n_roots = below(8) ? 1 + below(40) : 1 + below(MG_WT_MAX_ROOTS);
    s.n_atoms = below(8) ? below(40) : below(MG_WT_MAX_ATOMS + 1);
    s.n_code = below(200);
    s.n_resid = below(6);
    s.n_entries = below(4) ? below(9) : below(MG_AIM_MAX_ENTRIES + 1);
    s.n_pieces = below(30);
    s.n_srows = below(4) ? below(3) : below(MG_SUM_MAX_ROWS + 1);
    s.n_slots = below(4) ? below(3) : below(MG_UF_MAX_SLOTS + 1);
    s.n_funcs = below(4);
    s.n_cands = below(10);
    s.n_ukeys = below(5);
    s.n_urows = below(4) ? below(4) : below(MG_UF_MAX_ROWS + 1);
    s.mask_probe0 = below(3);
    s.n_probes = s.mask_probe0 + (s.n_roots + 255) / 256 + (s.n_atoms + 255) / 256 + s.n_resid +
                 s.n_srows + s.n_urows + below(3);
    return s;
}

static uint32_t* field(mg_walk_shape& s, uint32_t k) {
    uint32_t* f[] = {&s.n_leaves, &s.n_probes, &s.n_roots, &s.mask_probe0, &s.n_atoms, &s.n_code,
                     &s.n_resid, &s.n_entries, &s.n_pieces, &s.n_srows, &s.n_slots, &s.n_funcs,
                     &s.n_cands, &s.n_ukeys, &s.n_urows};
    return f[k % 15];
}

static void mutate(mg_walk_shape& s) {
    uint32_t* f = field(s, rnd());
    switch (below(5)) {
    case 0: *f = 0; break;
    case 1: *f += 1 + below(3); break;
    case 2: *f = 0xFFFFFFFFu - below(3); break;
    case 3: *f = below(2000); break;
    default: *f = rnd(); break;
    }
}

#define MAX_HOST_BYTES ((uint64_t)16 << 20)

// Lay the planned regions out in a buffer of exactly `bytes`; returns the
// bytes written.
static uint64_t materialise(const std::vector<mg_walk_shape>& shapes, uint32_t walkers,
                            uint32_t lanes, uint32_t max_rounds,
                            const std::vector<uint64_t>& off, uint64_t bytes, uint64_t leaf_w,
                            uint64_t probe_w) {
    const uint32_t n = (uint32_t)shapes.size();
    const uint64_t total = (uint64_t)walkers * lanes, w = walkers;
    uint8_t* buf = (uint8_t*)malloc(bytes ? bytes : 1);
    if (!buf) abort();
    memset(buf, 0, bytes);
    uint64_t written = 0;
    auto claim = [&](uint64_t at, uint64_t len) {
        if (at % 256) abort();                          // every region is aligned
        if (len && memchr(buf + at, 1, len)) abort();   // two regions overlap
        if (len) memset(buf + at, 1, len);
        written += len;
    };
    claim(off[MG_WB_DESCS], (uint64_t)n * sizeof(mg_pdesc));
    claim(off[MG_WB_JOBS], (uint64_t)n * sizeof(mg_walk_batch_job));
    claim(off[MG_WB_FROZEN], (uint64_t)n * 4);
    claim(off[MG_WB_STATES], w * n * sizeof(mg_walk_state));
    claim(off[MG_WB_ROOTBITS], (total + 63) / 64 * 8 * n);
    uint32_t max_leaves = 0, max_probes = 0;
    for (uint32_t g = 0; g < n; ++g) {
        const mg_walk_shape& s = shapes[g];
        max_leaves = s.n_leaves > max_leaves ? s.n_leaves : max_leaves;
        max_probes = s.n_probes > max_probes ? s.n_probes : max_probes;
        const uint64_t mwords = ((uint64_t)s.n_roots + 255) / 256 * 8 +
                                ((uint64_t)s.n_atoms + 255) / 256 * 8;
        const uint64_t len[MG_WB_JOB_REGIONS] = {
            w * s.n_leaves * 32, (uint64_t)s.n_leaves * sizeof(mg_leafgen), (uint64_t)s.n_roots * 4,
            (uint64_t)s.n_atoms * 4, (uint64_t)s.n_code * 4, (uint64_t)s.n_entries * 20,
            (uint64_t)s.n_pieces * 16, (uint64_t)s.n_entries * 32, (uint64_t)s.n_entries * 4,
            (uint64_t)s.n_slots * 8, (uint64_t)s.n_funcs * 12, (uint64_t)s.n_cands * 24,
            (uint64_t)s.n_ukeys * 32, w * max_rounds * 8, w * s.n_resid * 32,
            w * MG_AIM_LIVE_WORDS * 4, w * mwords * 4, w * s.n_urows * 32, w * s.n_srows * 32,
            w * s.n_slots * 4,
            // what the mutate kernel and the interpreter write for this job
            (uint64_t)s.n_leaves * 8 * total * 4, (uint64_t)s.n_probes * 8 * total * 4};
        for (uint32_t k = 0; k < MG_WB_JOB_REGIONS; ++k) claim(off[MG_WB_OFF(g, k)], len[k]);
    }
    // the strides are the batch's maxima, and job g's regions lie g strides on
    if (leaf_w * 4 < (uint64_t)max_leaves * 32 * total || leaf_w * 4 % 256) abort();
    if (probe_w * 4 < (uint64_t)max_probes * 32 * total || probe_w * 4 % 256) abort();
    for (uint32_t g = 0; g < n; ++g) {
        if (off[MG_WB_OFF(g, MG_WB_LEAVES)] != off[MG_WB_OFF(0, MG_WB_LEAVES)] + g * leaf_w * 4)
            abort();
        if (off[MG_WB_OFF(g, MG_WB_PROBES)] != off[MG_WB_OFF(0, MG_WB_PROBES)] + g * probe_w * 4)
            abort();
    }
    free(buf);
    return written;
}

// plan, and lay out what is accepted and small enough; true when planned
static bool drive(const std::vector<mg_walk_shape>& shapes, uint32_t n_jobs, uint32_t walkers,
                  uint32_t lanes, uint32_t max_rounds, unsigned long long* laid,
                  unsigned long long* bytes_laid) {
    // the table has room for the jobs given, as the ABI's has; n_jobs beyond
    // the cap is refused before anything is written
    std::vector<uint64_t> off(MG_WB_SHARED + shapes.size() * MG_WB_JOB_REGIONS);
    uint64_t bytes = 0, leaf_w = 0, probe_w = 0;
    if (!mg_walk_batch_plan(shapes.data(), n_jobs, walkers, lanes, max_rounds, off.data(), &bytes,
                            &leaf_w, &probe_w))
        return false;
    if (n_jobs != shapes.size()) abort();
    if (bytes % 256) abort();
    if (bytes <= MAX_HOST_BYTES) {
        *bytes_laid += materialise(shapes, walkers, lanes, max_rounds, off, bytes, leaf_w, probe_w);
        ++*laid;
    }
    return true;
}

int main(int argc, char** argv) {
    const long iterations = argc > 1 ? atol(argv[1]) : 2000;
    long valid_accepted = 0, valid_planned = 0, mutated = 0, mutated_accepted = 0,
         mutated_planned = 0, random_accepted = 0, random_planned = 0, shared_refused = 0;
    unsigned long long laid = 0, bytes_laid = 0;
    const uint32_t lane_counts[] = {1, 7, 16, 63, 64, 65, 257};
    for (long it = 0; it < iterations; ++it) {
        const uint32_t n = 1 + below(6), walkers = 1 + below(below(4) ? 3 : MG_WALK_MAX_WALKERS),
                       lanes = lane_counts[below(7)], rounds = 1 + below(40);
        std::vector<mg_walk_shape> jobs;
        bool ok = true;
        for (uint32_t g = 0; g < n; ++g) {
            jobs.push_back(valid());
            ok = ok && mg_walk_batch_shape_ok(jobs.back());
        }
        valid_accepted += ok;
        valid_planned += drive(jobs, n, walkers, lanes, rounds, &laid, &bytes_laid);
        for (int m = 0; m < 4; ++m) {
            std::vector<mg_walk_shape> u = jobs;
            mutate(u[below(n)]);
            ++mutated;
            bool all = true;
            for (const mg_walk_shape& s : u) all = all && mg_walk_batch_shape_ok(s);
            mutated_accepted += all;
            // the plan does not depend on the check: it must hold for any counts
            mutated_planned += drive(u, n, walkers, lanes, rounds, &laid, &bytes_laid);
        }
        std::vector<mg_walk_shape> r(n);
        bool all = true;
        for (mg_walk_shape& s : r) {
            for (uint32_t k = 0; k < 15; ++k) *field(s, k) = below(3) ? rnd() : below(300);
            all = all && mg_walk_batch_shape_ok(s);
        }
        random_accepted += all;
        random_planned += drive(r, n, below(2) ? walkers : MG_WALK_MAX_WALKERS,
                                below(2) ? lanes : MG_REPAIR_MAX_LANES, rounds, &laid,
                                &bytes_laid);
        // shared arguments out of range are refused whatever the shapes
        const uint32_t bad = below(6);
        const uint32_t bn = bad == 0 ? 0 : bad == 1 ? MG_WALK_BATCH_MAX_JOBS + 1 + below(1000) : n,
                       bw = bad == 2 ? (below(2) ? 0 : MG_WALK_MAX_WALKERS + 1 + below(100)) : walkers,
                       bl = bad == 3 ? (below(2) ? 0 : MG_REPAIR_MAX_LANES + 1 + below(100)) : lanes,
                       br = bad == 4 ? (below(2) ? 0 : MG_REPAIR_MAX_ROUNDS + 1 + below(100)) : rounds;
        const bool planned = drive(jobs, bn, bw, bl, br, &laid, &bytes_laid);
        if (planned != (bad == 5)) abort();
        shared_refused += !planned;
    }
    printf("{\"iterations\": %ld, \"valid_accepted\": %ld, \"valid_planned\": %ld, "
           "\"mutated\": %ld, \"mutated_accepted\": %ld, \"mutated_planned\": %ld, "
           "\"random_accepted\": %ld, \"random_planned\": %ld, \"shared_refused\": %ld, "
           "\"laid_out\": %llu, \"bytes_laid\": %llu}\n",
           iterations, valid_accepted, valid_planned, mutated, mutated_accepted, mutated_planned,
           random_accepted, random_planned, shared_refused, laid, bytes_laid);
    return 0;
}

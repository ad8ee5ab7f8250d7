// Sanitizer fuzz of the host side of mg_census_batch:
// csrc/mg_census_batch.h alone, the check of a job's counts
// (mg_census_shape_ok), the blocks rule (mg_census_batch_blocks) and the plan
// of the batch's device buffer with its chunk rule (mg_census_batch_plan).
// Random valid shapes, copies with one count mutated and shapes of random
// words go through them, with valid and random shared arguments.  Whatever
// the plan accepts at a size a host can allocate is laid out in a buffer of
// exactly the planned bytes: every region is written at the size the ABI
// uploads or lets the kernels write (what the counts imply), so a region that
// leaves the buffer is an ASan report, and a byte written twice — two regions
// that overlap — aborts.  Every refusal is put into words in a small buffer.
// Stand-alone: its own main, built with g++ -fsanitize=address,undefined
// (tests/test_census_batch_sanitize.py).
//
//   fuzz_census_batch [iterations]   prints one JSON line of counters

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mg_census_batch.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}
static uint32_t below(uint32_t n) { return n ? rnd() % n : 0; }

static mg_census_shape valid() {
    mg_census_shape s;
    s.n_roots = below(4) ? 1 + below(70) : 1 + below(MG_CENSUS_MAX_ROOTS);
    s.mask_probe0 = below(3);
    s.n_probes = s.mask_probe0 + (s.n_roots + 255) / 256 + below(3);
    return s;
}

static uint32_t* field(mg_census_shape& s, uint32_t k) {
    uint32_t* f[] = {&s.n_probes, &s.n_roots, &s.mask_probe0};
    return f[k % 3];
}

static void mutate(mg_census_shape& s) {
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
// bytes written.  Only shapes that passed the check name rows inside their
// region; the others claim the whole of what the interpreter writes.
static uint64_t materialise(const std::vector<mg_census_shape>& shapes, uint64_t lanes,
                            const std::vector<uint64_t>& off, uint64_t bytes, uint64_t count_w,
                            uint64_t probe_w) {
    const uint32_t n = (uint32_t)shapes.size();
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
    claim(off[MG_CB_DESCS], (uint64_t)n * sizeof(mg_pdesc));
    claim(off[MG_CB_JOBS], (uint64_t)n * sizeof(mg_census_batch_job));
    uint32_t max_probes = 0, max_roots = 0;
    for (uint32_t g = 0; g < n; ++g) {
        const mg_census_shape& s = shapes[g];
        max_probes = s.n_probes > max_probes ? s.n_probes : max_probes;
        max_roots = s.n_roots > max_roots ? s.n_roots : max_roots;
        // the job's own counter block, and what the interpreter writes for it
        claim(off[MG_CB_OFF(g, MG_CB_COUNTS)], (5 * (uint64_t)s.n_roots + 2) * 8);
        claim(off[MG_CB_OFF(g, MG_CB_PROBES)], (uint64_t)s.n_probes * 8 * lanes * 4);
        if (mg_census_shape_ok(s)) {
            // the rows the kernel reads end inside the region
            const uint64_t n_words = (s.n_roots + 31) / 32;
            if (((uint64_t)s.mask_probe0 * 8 + n_words) * lanes > probe_w) abort();
            if (mg_census_words(s.n_roots) > count_w) abort();
        }
    }
    // the strides are the batch's maxima, and job g's regions lie g strides on
    if (count_w * 8 < (5 * (uint64_t)max_roots + 2) * 8 || count_w * 8 % 256) abort();
    if (probe_w * 4 < (uint64_t)max_probes * 32 * lanes || probe_w * 4 % 256) abort();
    for (uint32_t g = 0; g < n; ++g) {
        if (off[MG_CB_OFF(g, MG_CB_COUNTS)] != off[MG_CB_OFF(0, MG_CB_COUNTS)] + g * count_w * 8)
            abort();
        if (off[MG_CB_OFF(g, MG_CB_PROBES)] != off[MG_CB_OFF(0, MG_CB_PROBES)] + g * probe_w * 4)
            abort();
    }
    if (off[MG_CB_OFF(0, MG_CB_PROBES)] + n * probe_w * 4 != bytes) abort();
    free(buf);
    return written;
}

struct tally {
    unsigned long long laid = 0, bytes_laid = 0, refused[MG_CB_OVERFLOW + 1] = {0};
};

// plan, word a refusal, and lay out what is accepted and small enough; the status
static int drive(const std::vector<mg_census_shape>& shapes, uint32_t n_jobs, uint64_t n_cand,
                 uint64_t chunk, tally* t) {
    // the table has room for the jobs given, as the ABI's has; n_jobs beyond
    // the cap is refused before anything is written
    std::vector<uint64_t> off(MG_CB_SHARED + shapes.size() * MG_CB_JOB_REGIONS);
    uint64_t bytes = 0, got = 0, need = 0, count_w = 0, probe_w = 0;
    const int st = mg_census_batch_plan(shapes.data(), n_jobs, n_cand, chunk, off.data(), &bytes,
                                        &got, &need, &count_w, &probe_w);
    std::vector<char> why(48, 'x');                     // shorter than some messages
    mg_census_batch_why(st, n_jobs, chunk, need, why.data(), why.size());
    if (!memchr(why.data(), 0, why.size())) abort();
    if (st < 0 || st > MG_CB_OVERFLOW) abort();
    ++t->refused[st];
    if (st != MG_CB_OK) {
        if ((st == MG_CB_CHUNK_BYTES || st == MG_CB_NO_FIT) && need <= MG_CENSUS_MAX_PROBE_BYTES)
            abort();
        return st;
    }
    if (n_jobs != shapes.size()) abort();
    if (bytes % 256 || got == 0 || got % 256 || (chunk && got != chunk)) abort();
    if (!chunk && got > MG_CENSUS_CHUNK) abort();
    // the probe regions of a whole chunk fit the cap ...
    uint32_t max_probes = 0;
    for (const mg_census_shape& s : shapes) max_probes = s.n_probes > max_probes ? s.n_probes : max_probes;
    const uint64_t lane_b = (uint64_t)max_probes * 32 * n_jobs;
    if (lane_b * got > MG_CENSUS_MAX_PROBE_BYTES) abort();
    // ... and with chunk 0 the next multiple of 256 would not, short of 2^16
    if (!chunk && got < MG_CENSUS_CHUNK && lane_b * (got + 256) <= MG_CENSUS_MAX_PROBE_BYTES) abort();
    const uint64_t lanes = n_cand < got ? n_cand : got;
    if (bytes <= MAX_HOST_BYTES) {
        t->bytes_laid += materialise(shapes, lanes, off, bytes, count_w, probe_w);
        ++t->laid;
    }
    return st;
}

int main(int argc, char** argv) {
    const long iterations = argc > 1 ? atol(argv[1]) : 2000;
    long valid_accepted = 0, valid_planned = 0, mutated = 0, mutated_accepted = 0,
         mutated_planned = 0, random_accepted = 0, random_planned = 0, shared_refused = 0,
         blocks_checked = 0;
    tally t;
    const uint64_t cands[] = {0, 1, 63, 64, 65, 255, 256, 257, 1000, 4096, 1 << 16};
    for (long it = 0; it < iterations; ++it) {
        const uint32_t n = 1 + below(below(8) ? 6 : MG_CENSUS_BATCH_MAX_JOBS);
        const uint64_t n_cand = cands[below(11)];
        const uint64_t chunk = below(3) ? 0 : 256u * (1 + below(8));
        std::vector<mg_census_shape> jobs;
        bool ok = true;
        for (uint32_t g = 0; g < n; ++g) {
            jobs.push_back(valid());
            ok = ok && mg_census_shape_ok(jobs.back());
        }
        valid_accepted += ok;
        // at most 8 probes x 256 jobs x 32 bytes x 2048 lanes: always within the cap
        valid_planned += drive(jobs, n, n_cand, chunk, &t) == MG_CB_OK;
        for (int m = 0; m < 4; ++m) {
            std::vector<mg_census_shape> u = jobs;
            mutate(u[below(n)]);
            ++mutated;
            bool all = true;
            for (const mg_census_shape& s : u) all = all && mg_census_shape_ok(s);
            mutated_accepted += all;
            // the plan does not depend on the check: it must hold for any counts
            mutated_planned += drive(u, n, n_cand, chunk, &t) == MG_CB_OK;
        }
        std::vector<mg_census_shape> r(n);
        bool all = true;
        for (mg_census_shape& s : r) {
            for (uint32_t k = 0; k < 3; ++k) *field(s, k) = below(3) ? rnd() : below(300);
            all = all && mg_census_shape_ok(s);
        }
        random_accepted += all;
        const uint64_t rc = below(2) ? chunk : ((uint64_t)rnd() << 32 | rnd()) & ~(uint64_t)255;
        random_planned += drive(r, n, below(2) ? n_cand : (uint64_t)rnd() << 21, rc, &t) == MG_CB_OK;
        // shared arguments out of range are refused whatever the shapes
        const uint32_t bad = below(4);
        const uint32_t bn = bad == 0 ? 0 : bad == 1 ? MG_CENSUS_BATCH_MAX_JOBS + 1 + below(1000) : n;
        const uint64_t bc = bad == 2 ? 256u * below(8) + 1 + below(255) : chunk;
        const int st = drive(jobs, bn, n_cand, bc, &t);
        if ((st == MG_CB_OK) != (bad == 3)) abort();
        if (bad < 2 && st != MG_CB_N_JOBS) abort();
        if (bad == 2 && st != MG_CB_CHUNK_MULTIPLE) abort();
        shared_refused += st != MG_CB_OK;
        // the blocks rule: at least one block, no more than tiles, the grid near the cap
        const uint64_t bn_cand = below(2) ? n_cand : ((uint64_t)rnd() << 20) + rnd();
        const uint32_t b = mg_census_batch_blocks(n, bn_cand);
        const uint64_t tiles = (bn_cand + 255) / 256;
        if (bn_cand == 0 ? b != 0 : (b < 1 || b > tiles || (uint64_t)b * n > MG_CENSUS_BATCH_GRID ||
                                     (b < tiles && (uint64_t)(b + 1) * n <= MG_CENSUS_BATCH_GRID)))
            abort();
        if (mg_census_batch_blocks(0, bn_cand) != 0) abort();
        ++blocks_checked;
    }
    printf("{\"iterations\": %ld, \"valid_accepted\": %ld, \"valid_planned\": %ld, "
           "\"mutated\": %ld, \"mutated_accepted\": %ld, \"mutated_planned\": %ld, "
           "\"random_accepted\": %ld, \"random_planned\": %ld, \"shared_refused\": %ld, "
           "\"blocks_checked\": %ld, \"laid_out\": %llu, \"bytes_laid\": %llu, "
           "\"refused_chunk_bytes\": %llu, \"refused_no_fit\": %llu, \"refused_overflow\": %llu}\n",
           iterations, valid_accepted, valid_planned, mutated, mutated_accepted, mutated_planned,
           random_accepted, random_planned, shared_refused, blocks_checked, t.laid, t.bytes_laid,
           t.refused[MG_CB_CHUNK_BYTES], t.refused[MG_CB_NO_FIT], t.refused[MG_CB_OVERFLOW]);
    return 0;
}

/* Device counter block of the verdict census (mg_census.hip, mg_census in
 * mg_api.cpp): u64 words, the sums first (zeroed before the first chunk),
 * then the minima (preset to ~0). */
#ifndef MG_CENSUS_H
#define MG_CENSUS_H

#include <stddef.h>
#include <stdint.h>

#define MG_CENSUS_MAX_ROOTS 1024u
/* best = failing roots << 53 | offset of the candidate from the census's
 * first index: 11 bits hold 0..1024 failing roots, so a census covers fewer
 * than 2^53 candidates */
#define MG_CENSUS_OFFSET_BITS 53

/* Candidates per census launch when the caller names none, and the largest
 * probe buffer one chunk may need (every probe of the loaded program has a
 * row set in it, written or not). */
#define MG_CENSUS_CHUNK (1ull << 16)
#define MG_CENSUS_MAX_PROBE_BYTES ((size_t)256 << 20)

#define MG_CENSUS_FN static inline __attribute__((always_inline))
#ifdef __HIPCC__
#undef MG_CENSUS_FN
#define MG_CENSUS_FN __host__ __device__ static inline __attribute__((always_inline))
#endif

MG_CENSUS_FN uint32_t mg_census_pass(uint32_t) { return 0; }
MG_CENSUS_FN uint32_t mg_census_first(uint32_t r) { return r; }
MG_CENSUS_FN uint32_t mg_census_sole(uint32_t r) { return 2 * r; }
MG_CENSUS_FN uint32_t mg_census_hist(uint32_t r) { return 3 * r; }             /* r + 1 words */
MG_CENSUS_FN uint32_t mg_census_sole_index(uint32_t r) { return 4 * r + 1; }   /* minima from here */
MG_CENSUS_FN uint32_t mg_census_best(uint32_t r) { return 5 * r + 1; }
MG_CENSUS_FN uint32_t mg_census_words(uint32_t r) { return 5 * r + 2; }

#endif

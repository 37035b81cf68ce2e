// The n-gram key of the device CIDEr-D scorer and its hash: ONE definition, included by cider.cpp (g++: builds the
// document-frequency table and the cooked references) and by cider_dev.hip (hipcc: builds the hypothesis keys and probes).
//
// An n-gram of order k <= 4 over the ids w0 .. w(k-1) is the 64-bit word whose 16-bit field j holds w_j + 1 for j < k and
// 0 for j >= k.  A used field is never 0, so the number of leading non-zero fields is the order: n-grams of different
// orders cannot collide, and 0 is no key at all - it marks an empty slot of the table.  Needs every id in [0, 65534].
#ifndef INSENTICAP_CIDER_KEY_H
#define INSENTICAP_CIDER_KEY_H

#include <stdint.h>

#if defined(__HIPCC__)
#define ISC_CIDER_HD __host__ __device__ __forceinline__
#else
#define ISC_CIDER_HD static inline
#endif

#define ISC_CIDER_MAX_ID 65534      /* the largest id a key can hold */
#define ISC_CIDER_MAX_ORDER 4

/* field j of a key for id w (the caller has checked 0 <= w <= ISC_CIDER_MAX_ID) */
ISC_CIDER_HD uint64_t isc_cider_field(int64_t w, int j) { return (uint64_t)((w + 1) & 0xFFFF) << (16 * j); }

ISC_CIDER_HD uint64_t isc_cider_key(const int64_t *w, int k) {
    uint64_t key = 0;
    for (int j = 0; j < k; ++j) key |= isc_cider_field(w[j], j);
    return key;
}

/* 64-bit finaliser (splitmix64); the home slot of a key is isc_cider_hash(key) & (capacity - 1), then linear probing */
ISC_CIDER_HD uint64_t isc_cider_hash(uint64_t key) {
    key ^= key >> 30;
    key *= 0xBF58476D1CE4E5B9ull;
    key ^= key >> 27;
    key *= 0x94D049BB133111EBull;
    key ^= key >> 31;
    return key;
}

#if defined(__HIPCC__)
/* Value of `v` in lane j of the wave, j wave-uniform (the device scorers hand keys round with it). */
__device__ __forceinline__ uint64_t lane_u64(uint64_t v, int j) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), j);
    return ((uint64_t)hi << 32) | lo;
}
#endif

/* One slot of the document-frequency table: 16 bytes.  key == 0: empty. */
typedef struct {
    uint64_t key;
    double log_df; /* log(max(1, df)): the `d` of counts2vec, formed on the host */
} isc_cider_slot;

#endif

// sid_hash.h -- the prefix hash of the semantic-id prefix index (csrc/sid_match.hip), shared with the beam step
// (csrc/beam_step.hip), which probes the same index.  A prefix of length h is hashed by seeding with kSidHashSeed,
// applying sid_hash_step to its ids in order and finishing with sid_hash_final; its slot in the table of length h is
// that value masked to slots_for(N) - 1.  Changing any bit here changes the index layout for every consumer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rqhip {

constexpr unsigned kSidHashSeed = 0x9747b28cu;

__device__ __forceinline__ unsigned sid_mix(unsigned h, unsigned v) {
    h ^= v + 0x9e3779b9u + (h << 6) + (h >> 2);
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    return h;
}

__device__ __forceinline__ unsigned sid_hash_step(unsigned h, int64_t v) {
    h = sid_mix(h, (unsigned)(unsigned long long)v);
    const unsigned hi = (unsigned)((unsigned long long)v >> 32);
    return hi ? sid_mix(h, hi ^ 0x5bd1e995u) : h;  // ids are small non-negative numbers: the high word is 0
}

__device__ __forceinline__ unsigned sid_hash_final(unsigned h) {
    h ^= h >> 16;
    h *= 0xc2b2ae35u;
    h ^= h >> 15;
    return h;
}

inline unsigned long long slots_for(long long N) {
    unsigned long long p = 64;
    const unsigned long long want = 2ull * (unsigned long long)(N > 0 ? N : 1);
    while (p < want) p <<= 1;
    return p;
}

}  // namespace rqhip

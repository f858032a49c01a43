// t5_dropout_hash.h -- the dropout decision the T5 kernels share (t5_attention.hip, t5_add_norm.hip): a pure function
// of a 64-bit seed and a 64-bit element index, documented at rqhip_t5_attention_fwd_train in include/rqhip.h and
// restated in torch integer operations by rqhip/ops.py:t5_attention_dropout_keep.  No mask is ever stored.
#pragma once

#include <hip/hip_runtime.h>

namespace rqhip {

// murmur3's 32-bit finaliser
__device__ __forceinline__ unsigned att_fmix32(unsigned h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// element idx is kept when its hash reaches thresh = round(p * 2^32)
__device__ __forceinline__ bool att_keep(unsigned long long seed, unsigned long long idx, unsigned thresh) {
    unsigned h = att_fmix32((unsigned)seed ^ (unsigned)idx);
    h = att_fmix32((h ^ (unsigned)(seed >> 32) ^ ((unsigned)(idx >> 32) * 0x85EBCA6Bu)) + 0x9E3779B9u);
    return h >= thresh;
}

}  // namespace rqhip

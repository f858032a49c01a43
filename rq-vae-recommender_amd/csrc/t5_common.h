// t5_common.h -- what the T5 kernel files share (t5_attention.hip, t5_add_norm.hip, t5_ffn.hip, sid_head_loss.hip,
// sid_embed.hip, t5_proj.hip): the vector types, the dropout decision, its threshold and its two scales, the wave
// reductions, the bf16 fragment helpers of the matrix kernels and the entry points' pointer checks.
// The matrix code that t5_ffn.hip and t5_proj.hip share beyond that (operand loaders, group step, chains): t5_matmul.h.
#pragma once

#include <math.h>

#include "rqhip_common.h"

namespace rqhip {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- dropout.  The decision is a pure function of a 64-bit seed and a 64-bit element index, documented at
// rqhip_t5_attention_fwd_train in include/rqhip.h and restated in torch integer operations by
// rqhip/ops.py:t5_attention_dropout_keep.  No mask is ever stored.

// murmur3's 32-bit finaliser
__device__ __forceinline__ unsigned fmix32(unsigned h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// element idx is kept when its hash reaches thresh = dropout_threshold(p)
__device__ __forceinline__ bool dropout_keep(unsigned long long seed, unsigned long long idx, unsigned thresh) {
    unsigned h = fmix32((unsigned)seed ^ (unsigned)idx);
    h = fmix32((h ^ (unsigned)(seed >> 32) ^ ((unsigned)(idx >> 32) * 0x85EBCA6Bu)) + 0x9E3779B9u);
    return h >= thresh;
}

inline bool dropout_p_valid(double p) { return p >= 0.0 && p < 1.0; }  // false for a NaN

// round(p * 2^32), at most 2^32 - 1; 0 = no dropout
inline unsigned dropout_threshold(double p) {
    const double t = nearbyint(p * 4294967296.0);
    return t >= 4294967295.0 ? 4294967295u : (unsigned)t;
}

// The scale 1 / (1 - p) of the kept elements exists in TWO roundings, which differ in the last bit at some p (0.15, 0.6,
// 0.8, 0.9; not at 0.1 or 0.5).  Each is part of its kernels' documented arithmetic (include/rqhip.h) and is pinned by
// tests/test_gpu_t5_dropout_scale.py: do not merge them.
//   t5_add_norm.hip, t5_ffn.hip: evaluated in double and rounded once
inline float dropout_scale_f64(double p) { return (float)(1.0 / (1.0 - p)); }
//   t5_attention.hip (forward and backward): p rounded to fp32 first, then an fp32 subtraction and an fp32 divide
inline float dropout_scale_f32(double p) { return 1.0f / (1.0f - (float)p); }

// ---- wave reductions: an xor butterfly over the 64 lanes with DESCENDING masks (32, 16, 8, 4, 2, 1); every lane ends
// with the same bits.  (beam_step.hip and gumbel.hip use ascending masks, another summation order: they stay apart.)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, RQ_WAVE);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, RQ_WAVE));
    return v;
}

// ---- the two arithmetics of the matrix kernels (t5_ffn.hip, t5_proj.hip; contracts in include/rqhip.h).  A lane holds
// the 8 terms 8 kq .. 8 kq + 7 of a group of 32 reduction terms for its row (A) and its column (B).
//   "fp32"  exact fp32: eight v_mfma_f32_16x16x4_f32, instruction e on term 8 kq + e of every k-slot kq (in the kernels)
//   "bf16"  each operand rounded to bf16 (nearest even, v_cvt_pk_bf16_f32), then ONE v_mfma_f32_16x16x32_bf16, whose
//           A / B fragment is exactly that holding: lane l supplies k = 8 (l >> 4) + j, j = 0 .. 7, of row / column
//           l & 15.  Products of two bf16 values are exact in fp32; the accumulation is fp32.  The helpers below.
// The C / D layout is the same for both: register r of lane (i, kq) is row 4 kq + r, column i.
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ bf16x8 pack_bf16x8(const float (&v)[8]) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (__bf16)v[e];
    return o;
}

// one group of 32 terms on already packed fragments
__device__ __forceinline__ f32x4 mma_group_bf16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// ---- packed rows (t5_attention.hip's packed kernels, rows_pack.hip)

// Group b of a packed tensor of n rows: rows lo .. lo + len - 1, by the cumulative table cu [groups + 1].  An entry
// outside [0, n] is clamped and a length beyond the padded bound cut (the rule of seq_batch.hip's offsets): a bad table
// gives an empty or a short group, never an address.
__device__ __forceinline__ void packed_group(const int *cu, long long b, long long n, int bound, long long &lo, int &len) {
    long long first = cu[b], end = cu[b + 1];
    first = first < 0 ? 0 : (first > n ? n : first);
    end = end < first ? first : (end > n ? n : end);
    lo = first;
    len = (int)(end - first > bound ? bound : end - first);
}

// ---- the entry points' pointer checks (a null pointer counts as aligned: the null check is a separate one)
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <class... P>
bool any_null(const P *...p) {
    return (... || !p);
}

template <class... P>
bool all_aligned16(const P *...p) {
    return (... && aligned16(p));
}

}  // namespace rqhip

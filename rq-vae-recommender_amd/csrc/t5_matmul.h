// t5_matmul.h -- the matrix code t5_ffn.hip and t5_proj.hip share: the constants, operand loaders, group step, chain
// close and fence of their arithmetic contract (include/rqhip.h, rqhip_t5_ffn_*) exist here once.  The two arithmetics themselves are in t5_common.h.
//
// Layout.  Exact fp32 on v_mfma_f32_16x16x4_f32, operand layout as csrc/mlp_small.hip: lane (i, kq) = (lane & 15,
// lane >> 4) supplies k-slot kq of row / column i, and of a GROUP of 32 reduction terms it holds the 8 terms 8 kq ..
// 8 kq + 7, so instruction e of a group consumes term 8 kq + e of every slot (chain order 0 8 16 24 1 9 17 25 ... 7 15
// 23 31 within a group).  The "bf16" arithmetic (template parameter BF) is one v_mfma_f32_16x16x32_bf16 per group on the
// same eight registers, rounded to bf16 and packed in front of it: loads, chains and stores do not change.
//
// Operands.  Where the reduction runs along a row of an operand as stored, a lane loads its row's 8 terms as two float4
// (load_a; load_b<false> for the weights of two 16-column tiles).  Where it runs down the columns of the weights
// (KN: the data gradients on the weights as stored) the lane loads, for each of its 8 terms, 2 consecutive columns and
// serves column 2 i + ct in column tile ct, a permutation the stores undo for free.  From a bf16 weight image
// (csrc/t5_images.hip), whose rows always hold the reduction terms, the 8 terms of a column tile are ONE 16-byte load,
// which is the instruction's B fragment as it stands.  Which lane serves a column does not enter its sum.
//
// Chains.  No chain is longer than kChainGroups groups (128 terms): a chain starts from +0, and a reduction's finished
// chains are added in ascending order from +0 (chain_close).  (One chain over all of d = 384 or F = 1024 passed the
// tests' gates, but with three to four times the operators' error in the worst cases; with chains of 128 the error is
// the operators' or less: profiles/t5_ffn_error.txt.)
//
// Weight gradients (the rule; the three kernels that apply it, t5_ffn_wgrad_kernel, t5_ffn_wgrad16_kernel and
// t5_proj_wgrad_kernel, keep their own bodies: a shared body, measured, cost the projections' kernel 1 % of its time).
// Every 32 x 32 tile of a weight gradient P^T . Q has one owning workgroup of 4 waves, which reduces over all N rows:
// blocks of kWgBlock rows, wave w takes the contiguous range of blocks [w nb / 4, (w + 1) nb / 4); within its range a
// wave starts a fresh chain every kWgFlush blocks (256 rows) and adds the finished chains in ascending order
// (chain_close; bounded chain length: the rounding error of a long row count grows with the number of chains, not of
// rows); the four waves' sums meet in LDS and are added in wave order.  No partial blocks in memory, no atomics, no
// reduction launch.  Under BF the lane's eight rows 4 ks + kq of a block are the elements j = ks of both fragments, a
// consistent permutation of the block's 32 rows.
#pragma once

#include "rqhip_common.h"
#include "t5_common.h"

namespace rqhip {

constexpr int kChainGroups = 4;      // groups of 32 terms per chain: 128 terms
constexpr int kWgBlock = 32;         // rows per block of the weight-gradient reduction
constexpr int kWgFlush = 8;          // blocks per chain

// keeps a step's loads together and in front of the previous step's matrix instructions (csrc/mlp_small.hip)
#define T5_FENCE __builtin_amdgcn_sched_barrier(0)

// one row's 8 terms of a group
__device__ __forceinline__ void load_a(const float *at, float (&a)[8]) {
    const f32x4 lo = *reinterpret_cast<const f32x4 *>(at);
    const f32x4 hi = *reinterpret_cast<const f32x4 *>(at + 4);
    a[0] = lo.x; a[1] = lo.y; a[2] = lo.z; a[3] = lo.w;
    a[4] = hi.x; a[5] = hi.y; a[6] = hi.z; a[7] = hi.w;
}

// the weight operand of one group for two 16-column tiles.  KN = false: `at` points at term 0 of the group in the row
// of tile 0's column, rows `ld` apart (tile 1: 16 rows on).  KN = true: `at` points at the lane's 2 columns in the row
// of the group's term 0, terms `ld` apart: the lane serves column 2 i + ct in column tile ct.
template <bool KN>
__device__ __forceinline__ void load_b(const float *at, size_t ld, float (&b)[2][8]) {
    if constexpr (KN) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const f32x2 v = *reinterpret_cast<const f32x2 *>(at + (size_t)e * ld);
            b[0][e] = v.x; b[1][e] = v.y;
        }
    } else {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) load_a(at + (size_t)(16 * ct) * ld, b[ct]);
    }
}

// the same operand from a bf16 image whose rows hold the reduction terms: `at` as for KN = false; the 16 bytes are the
// lane's fragment of a column tile
__device__ __forceinline__ void load_b(const __bf16 *at, size_t ld, bf16x8 (&b)[2]) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) b[ct] = *reinterpret_cast<const bf16x8 *>(at + (size_t)(16 * ct) * ld);
}

// one group of 32 terms.  BF: one instruction per tile on the same eight registers, rounded and packed pairwise
template <int RT, bool BF>
__device__ __forceinline__ void mma(const float (&a)[RT][8], const float (&b)[2][8], f32x4 (&acc)[RT][2]) {
    if constexpr (BF) {
        const bf16x8 b0 = pack_bf16x8(b[0]), b1 = pack_bf16x8(b[1]);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const bf16x8 ar = pack_bf16x8(a[rt]);
            acc[rt][0] = mma_group_bf16(ar, b0, acc[rt][0]);
            acc[rt][1] = mma_group_bf16(ar, b1, acc[rt][1]);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
                    acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt][e], b[ct][e], acc[rt][ct], 0, 0, 0);
    }
}

// the "bf16" arithmetic on weight fragments that come packed from an image
template <int RT, bool BF>
__device__ __forceinline__ void mma(const float (&a)[RT][8], const bf16x8 (&b)[2], f32x4 (&acc)[RT][2]) {
    static_assert(BF, "weight images belong to the bf16 arithmetic");
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const bf16x8 ar = pack_bf16x8(a[rt]);
        acc[rt][0] = mma_group_bf16(ar, b[0], acc[rt][0]);
        acc[rt][1] = mma_group_bf16(ar, b[1], acc[rt][1]);
    }
}

// a finished chain joins the sum of the chains before it; the next chain starts from +0
template <int RT>
__device__ __forceinline__ void chain_close(f32x4 (&sum)[RT][2], f32x4 (&run)[RT][2]) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[rt][ct][r] = sum[rt][ct][r] + run[rt][ct][r];
            run[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
}

}  // namespace rqhip

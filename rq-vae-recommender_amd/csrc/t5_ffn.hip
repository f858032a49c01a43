// t5_ffn.hip -- the T5 feed-forward body wo(dropout(relu(wi(x)))) as one launch forward and at most two backward
// (gfx950; modules/t5.py, ffn_impl = "hip"; semantics and arithmetic contract in include/rqhip.h).  The operand layout,
// the group order, the chain rule, the operand loaders and the weight-gradient rule are csrc/t5_matmul.h's, which
// csrc/t5_proj.hip uses too.
//
// Row kernel (forward, and backward kernel 1: the same structure with the weights in the other orientation).  A
// workgroup of 4 waves owns T rows; their x (backward: d_y) stays in LDS.  It walks F in chunks of 128 columns:
//   phase 1  wave w computes columns 32 w .. 32 w + 31 of the chunk (two 16-column tiles, T / 16 row tiles) over the
//            whole of d, applies the epilogue (forward: ReLU, store of h, dropout and scale; backward: the mask
//            h > 0 and keep * s, store of g) and writes the result into one of two LDS chunk buffers;
//   phase 2  wave w adds chunk . W2 into the accumulators of its column pairs q = w, w + 4, ... (32 output columns
//            each) -- they live in registers for the whole walk; y (d_x) is written once at the end.
// No chain is longer than 128 terms: phase 1 starts a fresh chain every 4 groups of d, phase 2 one per chunk, and the
// finished chains are added in ascending order.
// One barrier per chunk: chunk c + 1 goes into the other buffer, and nobody can still read that one (a wave passes
// chunk c's barrier only after every wave has finished phase 2 of chunk c - 1).
// The weights are read as stored: along their rows forward (wi [F, d] and wo [d, F]), down their columns backward (wo,
// then wi), where the lane serves column 2 i + ct in column tile ct -- a permutation the epilogues undo for free.
// Row-tile height: T = 16 up to 16384 rows, 32 above.  A workgroup streams all of wi and wo through L2 whatever T
// is, so T = 32 halves that traffic; but the model's shapes (5120 and 256 rows) are short of workgroups, not of L2
// bandwidth: 16-row tiles give 320 and 16 workgroups instead of 160 and 8 on 256 CUs.  The registers of the
// two-deep operand buffers leave one workgroup per CU at d = 384 (one wave per SIMD, which two independent
// accumulators per wave keep at the matrix pipe's issue rate).  T follows N alone, and the chains do not depend on T.
//
// Weight-gradient kernel (backward kernel 2): every 32 x 32 tile of d_wi and of d_wo has one owning workgroup, which
// reduces g^T . x, or d_y^T . hd, over all N rows by the weight-gradient rule of csrc/t5_matmul.h.  hd is recomputed
// from h and the seed as it is loaded.
//
// Second arithmetic, "bf16" (template parameter BF, entry points rqhip_t5_ffn_*_bf16; contract in include/rqhip.h): the
// same kernels with one v_mfma_f32_16x16x32_bf16 per group in place of the eight fp32 instructions.  Memory and LDS stay
// fp32: the rounding happens in registers, so h is stored unrounded and the chunk buffer holds fp32 hd / g.
//
// Weight images (template parameter IMG of the row kernel, with BF only; entry points rqhip_t5_ffn_*_bf16w): the weights
// come from bf16 images (csrc/t5_images.hip), which hold the values the "bf16" arithmetic rounds them to.  The reduction
// always runs along an image's rows -- forward wi16 [F, d] and wo16 [d, F], backward the TRANSPOSED images wo16t [F, d]
// and wi16t [d, F] -- so a lane's 8 terms of a column tile are ONE 16-byte load: no conversion, half the registers in
// the operand buffers, and the backward serves column 16 ct + i like the forward.  Every output has the bits of the BF arm.
//
// Saved activations in bf16 (template parameter ACT of the row kernel, with BF only; t5_ffn_wgrad16_kernel; entry points
// rqhip_t5_ffn_*_bf16a / _bf16wa): what the backward keeps of the forward, and what the row kernel hands the
// weight-gradient kernel, are blocked bf16 images (layout in include/rqhip.h) of the very operands the BF arm rounds in
// registers: hd16 = bf16(keep ? h * s : 0) and x16 forward, g16 and dy16 backward.  A tile's image is written from LDS
// (the staged rows; the chunk buffer after its barrier), 8 or 16 bytes per (column, kq).  The backward's active set is
// hd16 > 0, so neither backward kernel hashes a dropout decision, and the weight-gradient kernel's fragment of a column
// of a block -- rows 4 ks + kq as elements j = ks -- is ONE 16-byte load.  Same operands, same chains: the BF arm's bits.
#include <math.h>

#include <type_traits>

#include "rqhip_common.h"
#include "t5_common.h"
#include "t5_matmul.h"

namespace rqhip {

namespace {

constexpr int kFfnMaxD = 512, kFfnMaxF = 8192;
constexpr int kFfnChunk = 128;            // columns of F per step of the walk: 32 per wave
constexpr int kFfnLdh = kFfnChunk + 4;    // row stride of a chunk buffer in LDS
constexpr long long kFfnTallFrom = 16384; // rows above which the row tile is 32 high

bool ffn_supported(int d, int F) {
    return d >= 32 && d <= kFfnMaxD && d % 32 == 0 && F >= 32 && F <= kFfnMaxF && F % 32 == 0;
}

struct FfnRows {
    const float *x;            // forward: x [N, d]; backward: d_y [N, d]
    const float *w1, *w2;      // forward: wi [F, d], wo [d, F]; backward: wo, wi.  IMG: the bf16 images behind these
                               // pointers, forward wi16 [F, d], wo16 [d, F]; backward wo16t [F, d], wi16t [d, F]
    const float *h_in;         // backward: h [N, F]
    float *mid;                // forward: h (or null); backward: g (or null)
    float *out;                // forward: y; backward: d_x (null: phase 2 is skipped)
    __bf16 *x16;               // ACT: the blocked image of the staged rows (forward x16, backward dy16), or null.  ACT
                               // also makes `mid` the blocked image hd16 / g16 and `h_in` the image hd16
    const long long *seed;     // one int64 on the device (read only when th != 0)
    unsigned th;               // round(p * 2^32); 0 = no dropout
    float s;                   // 1 / (1 - p)
    long long N;
    int d, F;
};

template <int RT>
__device__ __forceinline__ void ffn_load_a(const float *base, int ld, int off, float (&a)[RT][8]) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) load_a(base + 16 * rt * ld + off, a[rt]);
}

// The blocked bf16 image of an activation [N, C] (include/rqhip.h): element (n, c) is number ((n >> 5) * C + c) * 32 +
// 8 * (n & 3) + ((n & 31) >> 2), so the rows 4 ks + kq of a block, ks = 0 .. 7, are 16 consecutive bytes per column.
// This writes the T = 16 RT rows from m0 (a multiple of T) of `ncols` columns from c0, fp32 in LDS with row stride ld:
// per (column, kq) the tile's rows 4 ks + kq are 4 (RT = 1: half a block) or 8 consecutive elements, one store.
template <int RT>
__device__ __forceinline__ void ffn_store_image(const float *src, int ld, int ncols, __bf16 *img, int C, int c0, long long m0,
                                                int t) {
    const int ks0 = (int)(m0 & 31) >> 2;      // the tile's first row of a k-slot within its block: 0, or 4 (RT = 1)
    __bf16 *base = img + ((size_t)(m0 >> 5) * C + c0) * 32 + ks0;
    for (int f = t; f < 4 * ncols; f += 256) {
        const int c = f >> 2, kq = f & 3;
        const float *col = src + kq * ld + c;
        std::conditional_t<RT == 1, bf16x4, bf16x8> v;
#pragma unroll
        for (int ks = 0; ks < 4 * RT; ++ks) v[ks] = (__bf16)col[4 * ks * ld];
        *reinterpret_cast<decltype(v) *>(base + (size_t)c * 32 + 8 * kq) = v;
    }
}

// RT: 16-row tiles per workgroup; NP: column pairs (32 output columns) per wave, >= ceil(d / 128); BF: the "bf16"
// arithmetic (memory, LDS and the epilogues stay fp32: the operands are rounded as the fragments are packed); IMG: the
// weights are bf16 images read along their rows (the backward's are the transposed ones); ACT: the saved activations
// are blocked bf16 images (FfnRows), and the backward's active set is hd16 > 0 without a dropout decision
template <int RT, int NP, bool BWD, bool BF, bool IMG = false, bool ACT = false>
__global__ __launch_bounds__(256) void t5_ffn_rows_kernel(const FfnRows p) {
    static_assert(BF || !IMG, "weight images belong to the bf16 arithmetic");
    static_assert(BF || !ACT, "bf16 saved activations belong to the bf16 arithmetic");
    constexpr bool KN = BWD && !IMG;               // the reduction runs down the columns of the weights as stored
    using WT = std::conditional_t<IMG, __bf16, float>;
    using WB = std::conditional_t<IMG, bf16x8[2], float[2][8]>;      // a group's weight operand for two column tiles
    const WT *w1 = reinterpret_cast<const WT *>(p.w1), *w2 = reinterpret_cast<const WT *>(p.w2);
    extern __shared__ __align__(16) float ffn_lds[];
    constexpr int T = 16 * RT;
    const int d = p.d, F = p.F, ldx = d + 4;
    float *xs = ffn_lds;                 // [T][d + 4]
    float *hs = ffn_lds + T * ldx;       // [2][T][kFfnLdh]
    const int t = threadIdx.x, lane = t & 63, i = lane & 15, kq = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const long long m0 = (long long)blockIdx.x * T;

    for (int f = t; f < T * (d >> 2); f += 256) {       // rows past the batch: a valid row is read, nothing is stored
        const int r = f / (d >> 2), c4 = f % (d >> 2);
        const long long row = m0 + r < p.N ? m0 + r : p.N - 1;
        *reinterpret_cast<f32x4 *>(xs + r * ldx + 4 * c4) = *reinterpret_cast<const f32x4 *>(p.x + (size_t)row * d + 4 * c4);
    }
    __syncthreads();
    if constexpr (ACT) {
        if (p.x16) ffn_store_image<RT>(xs, ldx, d, p.x16, d, 0, m0, t);
        if constexpr (BWD)
            if (!p.out && !p.mid) return;      // d_wo alone: dy16 was all it needed of this kernel
    }

    unsigned long long seed = 0ull;
    if constexpr (!(ACT && BWD))
        if (p.th) seed = (unsigned long long)*p.seed;
    const int npairs = d >> 5, ngd = d >> 5;
    f32x4 acc2[NP][RT][2];
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc2[q][rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

    // The weight operands come from L2 / HBM with about a microsecond of latency and one workgroup may have a CU to
    // itself (256 rows are 16 workgroups), so each phase keeps two loads' worth of them in registers: while the
    // matrix instructions of one round run, the next round's loads are in flight; a phase's first round is requested
    // before the other phase ends (phase 2's over the epilogue and the barrier, the next chunk's phase 1 over phase 2).
    constexpr int RG = 2;                          // groups per round of phase 1: two rounds are one chain
    static_assert(kChainGroups == 2 * RG, "a chain is closed after every second round");
    const int nr1 = (ngd + RG - 1) / RG;
    const size_t ld1 = KN ? (size_t)F : (size_t)d, ld2 = KN ? (size_t)d : (size_t)F;
    WB pb[2][RG];                                  // phase 1: two rounds
    WB qb[2][NP];                                  // phase 2: two groups
    auto load1 = [&](WB (&dst)[RG], int fw, int r) {
#pragma unroll
        for (int gg = 0; gg < RG; ++gg) {
            const int g = min(RG * r + gg, ngd - 1);      // past d: a valid group is read and not used
            const WT *at = KN ? w1 + (size_t)(32 * g + 8 * kq) * F + fw + 2 * i
                              : w1 + (size_t)(fw + i) * d + 32 * g + 8 * kq;
            if constexpr (IMG) load_b(at, ld1, dst[gg]);
            else load_b<KN>(at, ld1, dst[gg]);
        }
    };
    auto comp1 = [&](const WB (&src)[RG], int r, f32x4 (&run)[RT][2]) {
#pragma unroll
        for (int gg = 0; gg < RG; ++gg) {
            const int g = RG * r + gg;
            if (g < ngd) {
                float a[RT][8];
                ffn_load_a<RT>(xs + i * ldx + 8 * kq, ldx, 32 * g, a);
                mma<RT, BF>(a, src[gg], run);
            }
        }
    };
    auto load2 = [&](WB (&dst)[NP], int f0, int g) {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int pair = w + 4 * q;
            if (pair < npairs) {
                const WT *at = KN ? w2 + (size_t)(f0 + 32 * g + 8 * kq) * d + 32 * pair + 2 * i
                                  : w2 + (size_t)(32 * pair + i) * F + f0 + 32 * g + 8 * kq;
                if constexpr (IMG) load_b(at, ld2, dst[q]);
                else load_b<KN>(at, ld2, dst[q]);
            }
        }
    };
    auto comp2 = [&](const WB (&src)[NP], const float *hb, int g, f32x4 (&run)[NP][RT][2]) {
        float a[RT][8];
        ffn_load_a<RT>(hb + i * kFfnLdh + 8 * kq, kFfnLdh, 32 * g, a);
#pragma unroll
        for (int q = 0; q < NP; ++q)
            if (w + 4 * q < npairs) mma<RT, BF>(a, src[q], run[q]);
    };

    if (32 * w < F) load1(pb[0], 32 * w, 0);
    int buf = 0;
    for (int f0 = 0; f0 < F; f0 += kFfnChunk, buf ^= 1) {
        float *hb = hs + buf * T * kFfnLdh;
        const int fw = f0 + 32 * w;     // this wave's 32 columns of the chunk
        f32x4 acc1[RT][2], run1[RT][2];      // the sum of the finished chains; the running chain
        float hv[RT][2][4];                  // backward: h at the lane's elements of the chunk
        if (fw < F) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) acc1[rt][ct] = run1[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (BWD) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if constexpr (ACT) {
                            // row 16 rt + 4 kq + r of the tile is element 8 r + (that row >> 2) of its column's block;
                            // rows past N are unspecified there and feed rows that are never stored
                            const __bf16 *hr = reinterpret_cast<const __bf16 *>(p.h_in) + ((size_t)(m0 >> 5) * F + fw) * 32 +
                                               8 * r + (((int)(m0 & 31) + 16 * rt) >> 2) + kq;
                            hv[rt][0][r] = (float)hr[(size_t)(KN ? 2 * i : i) * 32];
                            hv[rt][1][r] = (float)hr[(size_t)(KN ? 2 * i + 1 : 16 + i) * 32];
                        } else {
                            const long long grow = m0 + 16 * rt + 4 * kq + r;
                            const float *hr = p.h_in + (size_t)(grow < p.N ? grow : p.N - 1) * F + fw;
                            if constexpr (KN) {
                                const f32x2 v = *reinterpret_cast<const f32x2 *>(hr + 2 * i);
                                hv[rt][0][r] = v.x; hv[rt][1][r] = v.y;
                            } else {
                                hv[rt][0][r] = hr[i]; hv[rt][1][r] = hr[16 + i];
                            }
                        }
                    }
            }
            for (int r = 0; r < nr1; r += 2) {
                if (r + 1 < nr1) load1(pb[1], fw, r + 1);
                T5_FENCE; comp1(pb[0], r, run1); T5_FENCE;
                if (r + 1 < nr1) {
                    if (r + 2 < nr1) load1(pb[0], fw, r + 2);
                    T5_FENCE; comp1(pb[1], r + 1, run1); T5_FENCE;
                }
                chain_close<RT>(acc1, run1);      // rounds r and r + 1: 4 groups
            }
        }
        if (p.out) load2(qb[0], f0, 0);
        T5_FENCE;
        if (fw < F) {
            // acc1[rt][ct][r]: row 16 rt + 4 kq + r; column 16 ct + i (forward, images) or 2 i + ct (backward) of the wave's 32
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * rt + 4 * kq + r, lc = 32 * w + (KN ? 2 * i + ct : 16 * ct + i);
                        const long long grow = m0 + row;
                        const unsigned long long f = (unsigned long long)(f0 + lc);
                        float v = acc1[rt][ct][r];
                        if constexpr (!BWD) {
                            v = v <= 0.f ? 0.f : v;      // +0 for every pre-activation <= 0; a NaN stays a NaN
                            if constexpr (!ACT)
                                if (p.mid && grow < p.N) p.mid[(size_t)grow * F + f] = v;
                            if (p.th) v = dropout_keep(seed, (unsigned long long)grow * F + f, p.th) ? v * p.s : 0.f;
                        } else {
                            bool on = hv[rt][ct][r] > 0.f;
                            if (p.th) {
                                if constexpr (!ACT)      // ACT: hd16 > 0 is already h > 0 and keep
                                    on = on && dropout_keep(seed, (unsigned long long)(grow < p.N ? grow : p.N - 1) * F + f, p.th);
                                v = v * p.s;
                            }
                            v = on ? v : 0.f;
                            if constexpr (!ACT)
                                if (p.mid && grow < p.N) p.mid[(size_t)grow * F + f] = v;
                        }
                        hb[row * kFfnLdh + lc] = v;
                    }
        }
        __syncthreads();
        if constexpr (ACT)      // the chunk's hd (backward: g) as its image; the buffer is not rewritten before the next barrier
            if (p.mid)
                ffn_store_image<RT>(hb, kFfnLdh, F - f0 < kFfnChunk ? F - f0 : kFfnChunk, reinterpret_cast<__bf16 *>(p.mid), F,
                                    f0, m0, t);
        if (fw + kFfnChunk < F) load1(pb[0], fw + kFfnChunk, 0);
        if (p.out) {
            const int ng = (F - f0 < kFfnChunk ? F - f0 : kFfnChunk) >> 5;
            f32x4 run2[NP][RT][2];               // this chunk's chains
#pragma unroll
            for (int q = 0; q < NP; ++q)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) run2[q][rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int g = 0; g < ng; g += 2) {
                if (g + 1 < ng) load2(qb[1], f0, g + 1);
                T5_FENCE; comp2(qb[0], hb, g, run2); T5_FENCE;
                if (g + 1 < ng) {
                    if (g + 2 < ng) load2(qb[0], f0, g + 2);
                    T5_FENCE; comp2(qb[1], hb, g + 1, run2); T5_FENCE;
                }
            }
#pragma unroll
            for (int q = 0; q < NP; ++q) chain_close<RT>(acc2[q], run2[q]);
        }
    }
    if (!p.out) return;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int pair = w + 4 * q;
        if (pair >= npairs) continue;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long grow = m0 + 16 * rt + 4 * kq + r;
                if (grow >= p.N) continue;
                float *o = p.out + (size_t)grow * d + 32 * pair;
                if constexpr (KN) {
                    *reinterpret_cast<f32x2 *>(o + 2 * i) = f32x2{acc2[q][rt][0][r], acc2[q][rt][1][r]};
                } else {
                    o[i] = acc2[q][rt][0][r];
                    o[16 + i] = acc2[q][rt][1][r];
                }
            }
    }
}

struct FfnWgrad {
    const float *g, *x;        // d_wi [F, d] = g^T . x
    const float *dy, *h;       // d_wo [d, F] = d_y^T . hd, hd = keep ? h * s : 0
    float *d_wi, *d_wo;        // either may be null
    const long long *seed;
    unsigned th;
    float s;
    long long N;
    int d, F;
    int tiles_wi;              // workgroups [0, tiles_wi) own d_wi's tiles, the rest d_wo's
};

// BF: the "bf16" arithmetic; the lane's eight rows 4 ks + kq of a block are the elements j = ks of both fragments
template <bool BF>
__global__ __launch_bounds__(256) void t5_ffn_wgrad_kernel(const FfnWgrad p) {
    __shared__ float red[4 * 32 * 33];
    const int t = threadIdx.x, lane = t & 63, i = lane & 15, kq = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    int tile = blockIdx.x;
    const bool is_wo = tile >= p.tiles_wi;
    if (is_wo) tile -= p.tiles_wi;
    // out [rows of P's columns, columns of Q's columns] = sum_n P[n][a0 + .] Q[n][b0 + .]
    const float *P = is_wo ? p.dy : p.g, *Q = is_wo ? p.h : p.x;
    const int lp = is_wo ? p.d : p.F, lq = is_wo ? p.F : p.d;
    float *out = is_wo ? p.d_wo : p.d_wi;
    const int a0 = 32 * (tile / (lq >> 5)), b0 = 32 * (tile % (lq >> 5));
    const bool drop = is_wo && p.th != 0;
    const unsigned long long seed = drop ? (unsigned long long)*p.seed : 0ull;

    const long long nb = (p.N + kWgBlock - 1) / kWgBlock;
    const long long lo = w * nb / 4, hi = (w + 1) * nb / 4;
    f32x4 tot[2][2], acc[2][2];
#pragma unroll
    for (int at = 0; at < 2; ++at)
#pragma unroll
        for (int bt = 0; bt < 2; ++bt) tot[at][bt] = acc[at][bt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *pp = P + a0 + 2 * i, *qp = Q + b0 + 2 * i;
    // lane (i, kq): row 4 ks + kq of block b, columns 2 i and 2 i + 1; past the batch a valid row is read and counts as zero
    auto load = [&](long long b, f32x2 (&pa)[8], f32x2 (&qb)[8]) {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const long long n = b * kWgBlock + 4 * ks + kq;
            const long long nn = n < p.N ? n : p.N - 1;
            pa[ks] = *reinterpret_cast<const f32x2 *>(pp + (size_t)nn * lp);
            qb[ks] = *reinterpret_cast<const f32x2 *>(qp + (size_t)nn * lq);
        }
    };
    auto comp = [&](long long b, f32x2 (&pa)[8], f32x2 (&qb)[8]) {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const long long n = b * kWgBlock + 4 * ks + kq;
            if (drop) {
                const unsigned long long e = (unsigned long long)n * p.F + (unsigned long long)(b0 + 2 * i);
                qb[ks].x = dropout_keep(seed, e, p.th) ? qb[ks].x * p.s : 0.f;
                qb[ks].y = dropout_keep(seed, e + 1, p.th) ? qb[ks].y * p.s : 0.f;
            }
            if (n >= p.N) pa[ks] = qb[ks] = f32x2{0.f, 0.f};
        }
        if constexpr (BF) {
            bf16x8 fa[2], fb[2];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                fa[0][ks] = (__bf16)pa[ks].x; fa[1][ks] = (__bf16)pa[ks].y;
                fb[0][ks] = (__bf16)qb[ks].x; fb[1][ks] = (__bf16)qb[ks].y;
            }
#pragma unroll
            for (int at = 0; at < 2; ++at)
#pragma unroll
                for (int bt = 0; bt < 2; ++bt) acc[at][bt] = mma_group_bf16(fa[at], fb[bt], acc[at][bt]);
        } else {
#pragma unroll
            for (int ks = 0; ks < 8; ++ks)
#pragma unroll
                for (int at = 0; at < 2; ++at)
#pragma unroll
                    for (int bt = 0; bt < 2; ++bt)
                        acc[at][bt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[ks][at], qb[ks][bt], acc[at][bt], 0, 0, 0);
        }
        if (((b - lo) & (kWgFlush - 1)) == kWgFlush - 1) chain_close<2>(tot, acc);
    };
    f32x2 pa0[8], qb0[8], pa1[8], qb1[8];      // two blocks: the next one's loads are in flight over this one's instructions
    if (lo < hi) load(lo, pa0, qb0);
    for (long long b = lo; b < hi; b += 2) {
        if (b + 1 < hi) load(b + 1, pa1, qb1);
        T5_FENCE; comp(b, pa0, qb0); T5_FENCE;
        if (b + 1 < hi) {
            if (b + 2 < hi) load(b + 2, pa0, qb0);
            T5_FENCE; comp(b + 1, pa1, qb1); T5_FENCE;
        }
    }
    // acc[at][bt][r]: row 2 (4 kq + r) + at, column 2 i + bt of the tile (the lanes' own column pairs on both sides)
    float *mine = red + w * 32 * 33;
#pragma unroll
    for (int at = 0; at < 2; ++at)
#pragma unroll
        for (int bt = 0; bt < 2; ++bt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                mine[(2 * (4 * kq + r) + at) * 33 + 2 * i + bt] = tot[at][bt][r] + acc[at][bt][r];
    __syncthreads();
    for (int f = t; f < 32 * 32; f += 256) {
        const int row = f >> 5, col = f & 31;
        float v = red[row * 33 + col];
#pragma unroll
        for (int k = 1; k < 4; ++k) v = v + red[k * 32 * 33 + row * 33 + col];
        out[(size_t)(a0 + row) * lq + b0 + col] = v;
    }
}

struct FfnWgrad16 {
    const __bf16 *g, *x;       // blocked images: d_wi [F, d] = g^T . x
    const __bf16 *dy, *h;      // d_wo [d, F] = d_y^T . hd, h the image hd16
    float *d_wi, *d_wo;        // either may be null
    long long N;
    int d, F;
    int tiles_wi;
};

// t5_ffn_wgrad_kernel<true> on blocked bf16 images: the same tiles, blocks, chains, wave ranges and sums, and the same
// rows 4 ks + kq as elements j = ks -- which the image stores as the lane's 16 bytes of a column.  Lane (i, kq) serves
// columns 16 at + i of P's 32 and 16 bt + i of Q's: four 16-byte loads per block, contiguous over the wave, no
// conversion and no dropout decision (hd16 holds hd).  Which lane serves a column does not enter its sum.
__global__ __launch_bounds__(256) void t5_ffn_wgrad16_kernel(const FfnWgrad16 p) {
    __shared__ float red[4 * 32 * 33];
    const int t = threadIdx.x, lane = t & 63, i = lane & 15, kq = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    int tile = blockIdx.x;
    const bool is_wo = tile >= p.tiles_wi;
    if (is_wo) tile -= p.tiles_wi;
    const __bf16 *P = is_wo ? p.dy : p.g, *Q = is_wo ? p.h : p.x;
    const int lp = is_wo ? p.d : p.F, lq = is_wo ? p.F : p.d;
    float *out = is_wo ? p.d_wo : p.d_wi;
    const int a0 = 32 * (tile / (lq >> 5)), b0 = 32 * (tile % (lq >> 5));

    const long long nb = (p.N + kWgBlock - 1) / kWgBlock;
    const long long lo = w * nb / 4, hi = (w + 1) * nb / 4;
    f32x4 tot[2][2], acc[2][2];
#pragma unroll
    for (int at = 0; at < 2; ++at)
#pragma unroll
        for (int bt = 0; bt < 2; ++bt) tot[at][bt] = acc[at][bt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const __bf16 *pp = P + (size_t)(a0 + i) * 32 + 8 * kq, *qp = Q + (size_t)(b0 + i) * 32 + 8 * kq;
    // fr[0], fr[1]: P's column tiles; fr[2], fr[3]: Q's
    auto load = [&](long long b, bf16x8 (&fr)[4]) {
        const __bf16 *pb = pp + (size_t)b * lp * 32, *qb = qp + (size_t)b * lq * 32;
        fr[0] = *reinterpret_cast<const bf16x8 *>(pb);
        fr[1] = *reinterpret_cast<const bf16x8 *>(pb + 16 * 32);
        fr[2] = *reinterpret_cast<const bf16x8 *>(qb);
        fr[3] = *reinterpret_cast<const bf16x8 *>(qb + 16 * 32);
    };
    auto comp = [&](long long b, bf16x8 (&fr)[4]) {
        if ((b + 1) * kWgBlock > p.N) {      // the last block: rows past the batch are unspecified in memory and count as zero
#pragma unroll
            for (int ks = 0; ks < 8; ++ks)
                if (b * kWgBlock + 4 * ks + kq >= p.N) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) fr[k][ks] = (__bf16)0.f;
                }
        }
#pragma unroll
        for (int at = 0; at < 2; ++at)
#pragma unroll
            for (int bt = 0; bt < 2; ++bt) acc[at][bt] = mma_group_bf16(fr[at], fr[2 + bt], acc[at][bt]);
        if (((b - lo) & (kWgFlush - 1)) == kWgFlush - 1) chain_close<2>(tot, acc);
    };
    bf16x8 f0[4], f1[4];      // two blocks: the next one's loads are in flight over this one's instructions
    if (lo < hi) load(lo, f0);
    for (long long b = lo; b < hi; b += 2) {
        if (b + 1 < hi) load(b + 1, f1);
        T5_FENCE; comp(b, f0); T5_FENCE;
        if (b + 1 < hi) {
            if (b + 2 < hi) load(b + 2, f0);
            T5_FENCE; comp(b + 1, f1); T5_FENCE;
        }
    }
    // acc[at][bt][r]: row 16 at + 4 kq + r, column 16 bt + i of the tile
    float *mine = red + w * 32 * 33;
#pragma unroll
    for (int at = 0; at < 2; ++at)
#pragma unroll
        for (int bt = 0; bt < 2; ++bt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                mine[(16 * at + 4 * kq + r) * 33 + 16 * bt + i] = tot[at][bt][r] + acc[at][bt][r];
    __syncthreads();
    for (int f = t; f < 32 * 32; f += 256) {
        const int row = f >> 5, col = f & 31;
        float v = red[row * 33 + col];
#pragma unroll
        for (int k = 1; k < 4; ++k) v = v + red[k * 32 * 33 + row * 33 + col];
        out[(size_t)(a0 + row) * lq + b0 + col] = v;
    }
}

int ffn_row_tiles(long long N) { return N > kFfnTallFrom ? 2 : 1; }

// The checks the entry points share; `who` names the entry point in the message.
int ffn_check(const char *who, int64_t N, int d, int F, double p) {
    if (N < 0 || d < 1 || F < 1) {
        set_error("%s: bad sizes (N=%lld, d=%d, F=%d)", who, (long long)N, d, F);
        return RQHIP_EARG;
    }
    if (!dropout_p_valid(p)) {
        set_error("%s: dropout probability p=%g outside 0 <= p < 1", who, p);
        return RQHIP_EARG;
    }
    if (!ffn_supported(d, F)) {
        set_error("%s: d=%d, F=%d: only multiples of 32 with 32 <= d <= %d and 32 <= F <= %d are implemented", who, d, F,
                  kFfnMaxD, kFfnMaxF);
        return RQHIP_EUNSUPPORTED;
    }
    if (N / 16 >= (1ll << 31) - 1) {
        set_error("%s: N=%lld exceeds 16 rows per workgroup of a 2^31 grid", who, (long long)N);
        return RQHIP_EUNSUPPORTED;
    }
    return RQHIP_OK;
}

template <int RT, int NP, bool BWD, bool BF, bool IMG, bool ACT>
int ffn_rows_launch(const FfnRows &p, hipStream_t s) {
    static LdsGrant grant;
    constexpr int T = 16 * RT;
    const int bytes = (T * (p.d + 4) + 2 * T * kFfnLdh) * (int)sizeof(float);
    // granted once per device: the most this instantiation can ask for (d <= 128 NP)
    constexpr int most = (T * (128 * NP + 4) + 2 * T * kFfnLdh) * (int)sizeof(float);
    RQ_RETURN_IF_HIP(grant.ensure(reinterpret_cast<const void *>(t5_ffn_rows_kernel<RT, NP, BWD, BF, IMG, ACT>), most));
    hipLaunchKernelGGL((t5_ffn_rows_kernel<RT, NP, BWD, BF, IMG, ACT>), dim3((unsigned)((p.N + T - 1) / T)), dim3(256), (size_t)bytes, s, p);
    RQ_CHECK_LAUNCH("t5_ffn_rows_kernel");
    return RQHIP_OK;
}

template <bool BWD, bool BF, bool IMG, bool ACT = false>
int ffn_rows(const FfnRows &p, hipStream_t s) {
    const int np = (p.d / 32 + 3) / 4, rt = ffn_row_tiles(p.N);
    // The "bf16" backward at d > 384 keeps 16-row tiles at every N: its 32-row instantiation would spill to scratch
    // (so does the fp32 one, 44 bytes per lane, which stays as it is).  The tile height changes no bit.  The image
    // arm follows the same plan, and so does the arm with bf16 saved activations.
    constexpr bool kShortOnly = BF && BWD;
    if (rt == 1 || (kShortOnly && np == 4)) {
        if (np == 1) return ffn_rows_launch<1, 1, BWD, BF, IMG, ACT>(p, s);
        if (np == 2) return ffn_rows_launch<1, 2, BWD, BF, IMG, ACT>(p, s);
        if (np == 3) return ffn_rows_launch<1, 3, BWD, BF, IMG, ACT>(p, s);
        return ffn_rows_launch<1, 4, BWD, BF, IMG, ACT>(p, s);
    }
    if (np == 1) return ffn_rows_launch<2, 1, BWD, BF, IMG, ACT>(p, s);
    if (np == 2) return ffn_rows_launch<2, 2, BWD, BF, IMG, ACT>(p, s);
    if (np == 3) return ffn_rows_launch<2, 3, BWD, BF, IMG, ACT>(p, s);
    if constexpr (!kShortOnly) return ffn_rows_launch<2, 4, BWD, BF, IMG, ACT>(p, s);
    return RQHIP_EUNSUPPORTED;      // not reached: np == 4 left above
}

}  // namespace

}  // namespace rqhip

using namespace rqhip;

extern "C" int rqhip_t5_ffn_supported(int d, int F) { return ffn_supported(d, F) ? 1 : 0; }

extern "C" size_t rqhip_t5_ffn_act_image_bytes(int64_t N, int C) {
    if (N < 0 || C < 32 || C % 32) return 0;
    return (size_t)((N + kWgBlock - 1) / kWgBlock) * (size_t)C * kWgBlock * sizeof(rqhip_bf16_t);
}

extern "C" size_t rqhip_t5_ffn_bwd_bf16a_workspace_bytes(int64_t N, int d, int F) {
    if (N < 0 || !ffn_supported(d, F)) return 0;
    return rqhip_t5_ffn_act_image_bytes(N, d) + rqhip_t5_ffn_act_image_bytes(N, F);
}

extern "C" size_t rqhip_t5_ffn_bwd_workspace_bytes(int64_t N, int d, int F) {
    if (N < 0 || !ffn_supported(d, F)) return 0;
    return (size_t)N * (size_t)F * sizeof(float);
}

namespace {

// the entry points of both arithmetics; `who` names the one called in the messages.  IMG: wi and wo are the bf16 images
// the call reads (forward wi16, wo16; backward wo16t, wi16t, passed in the places of wo and wi)
// ACT: h is the blocked bf16 image hd16 behind that pointer and x16 the image of x (either may be null: not stored)
template <bool BF, bool IMG = false, bool ACT = false>
int ffn_fwd(const char *who, const float *x, const float *wi, const float *wo, int64_t N, int d, int F, double p,
            const int64_t *seed, float *y, float *h, rqhip_stream_t stream, rqhip_bf16_t *x16 = nullptr) {
    const int rc = ffn_check(who, N, d, F, p);
    if (rc != RQHIP_OK) return rc;
    if (N == 0) return RQHIP_OK;
    const unsigned th = dropout_threshold(p);
    if (any_null(x, wi, wo, y)) {
        set_error("%s: null pointer (x, wi, wo, y)", who);
        return RQHIP_EARG;
    }
    if (th && !seed) {
        set_error("%s: dropout (p=%g) needs the seed, a one-element int64 device pointer", who, p);
        return RQHIP_EARG;
    }
    if (!all_aligned16(x, wi, wo, y, h, x16)) {
        set_error(ACT ? "%s: x, wi, wo, y, hd16 and x16 must be 16-byte aligned" : "%s: x, wi, wo, y and h must be 16-byte aligned", who);
        return RQHIP_EARG;
    }
    FfnRows a;
    a.x = x, a.w1 = wi, a.w2 = wo, a.h_in = nullptr, a.mid = h, a.out = y, a.x16 = reinterpret_cast<__bf16 *>(x16);
    a.seed = reinterpret_cast<const long long *>(seed), a.th = th, a.s = dropout_scale_f64(p);
    a.N = N, a.d = d, a.F = F;
    return ffn_rows<false, BF, IMG, ACT>(a, reinterpret_cast<hipStream_t>(stream));
}

template <bool BF, bool IMG = false>
int ffn_bwd(const char *who, const float *x, const float *wi, const float *wo, const float *h, const float *d_y, int64_t N,
            int d, int F, double p, const int64_t *seed, float *d_x, float *d_wi, float *d_wo, void *workspace,
            rqhip_stream_t stream) {
    const int rc = ffn_check(who, N, d, F, p);
    if (rc != RQHIP_OK) return rc;
    if (N == 0 || (!d_x && !d_wi && !d_wo)) return RQHIP_OK;
    const unsigned th = dropout_threshold(p);
    if (any_null(x, wi, wo, h, d_y)) {
        set_error("%s: null pointer (x, wi, wo, h, d_y)", who);
        return RQHIP_EARG;
    }
    if (th && !seed) {
        set_error("%s: dropout (p=%g) needs the seed, a one-element int64 device pointer", who, p);
        return RQHIP_EARG;
    }
    if (d_wi && !workspace) {
        set_error("%s: d_wi needs a workspace of rqhip_t5_ffn_bwd_workspace_bytes(N, d, F) = %zu bytes", who,
                  rqhip_t5_ffn_bwd_workspace_bytes(N, d, F));
        return RQHIP_EWORKSPACE;
    }
    if (!all_aligned16(x, wi, wo, h, d_y, d_x, d_wi, d_wo, workspace)) {
        set_error("%s: x, wi, wo, h, d_y, d_x, d_wi, d_wo and the workspace must be 16-byte aligned", who);
        return RQHIP_EARG;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float *g = d_wi ? reinterpret_cast<float *>(workspace) : nullptr;
    if (d_x || d_wi) {
        FfnRows a;
        a.x = d_y, a.w1 = wo, a.w2 = wi, a.h_in = h, a.mid = g, a.out = d_x, a.x16 = nullptr;
        a.seed = reinterpret_cast<const long long *>(seed), a.th = th, a.s = dropout_scale_f64(p);
        a.N = N, a.d = d, a.F = F;
        const int rc1 = ffn_rows<true, BF, IMG>(a, s);
        if (rc1 != RQHIP_OK) return rc1;
    }
    if (d_wi || d_wo) {
        FfnWgrad q;
        q.g = g, q.x = x, q.dy = d_y, q.h = h, q.d_wi = d_wi, q.d_wo = d_wo;
        q.seed = reinterpret_cast<const long long *>(seed), q.th = th, q.s = dropout_scale_f64(p);
        q.N = N, q.d = d, q.F = F;
        const int tiles = (d / 32) * (F / 32);
        q.tiles_wi = d_wi ? tiles : 0;
        hipLaunchKernelGGL(t5_ffn_wgrad_kernel<BF>, dim3((unsigned)(q.tiles_wi + (d_wo ? tiles : 0))), dim3(256), 0, s, q);
        RQ_CHECK_LAUNCH("t5_ffn_wgrad_kernel");
    }
    return RQHIP_OK;
}

// the backward on bf16 saved activations.  The workspace holds dy16 and, behind it, g16: the row kernel writes both
// and the weight-gradient kernel reads them.  wi, wo: as ffn_bwd's (IMG: the transposed images)
template <bool IMG>
int ffn_bwd_act(const char *who, const rqhip_bf16_t *x16, const float *wi, const float *wo, const rqhip_bf16_t *hd16,
                const float *d_y, int64_t N, int d, int F, double p, float *d_x, float *d_wi, float *d_wo, void *workspace,
                rqhip_stream_t stream) {
    const int rc = ffn_check(who, N, d, F, p);
    if (rc != RQHIP_OK) return rc;
    if (N == 0 || (!d_x && !d_wi && !d_wo)) return RQHIP_OK;
    if (any_null(x16, wi, wo, hd16, d_y)) {
        set_error("%s: null pointer (x16, wi, wo, hd16, d_y)", who);
        return RQHIP_EARG;
    }
    if ((d_wi || d_wo) && !workspace) {
        set_error("%s: a weight gradient needs a workspace of rqhip_t5_ffn_bwd_bf16a_workspace_bytes(N, d, F) = %zu bytes", who,
                  rqhip_t5_ffn_bwd_bf16a_workspace_bytes(N, d, F));
        return RQHIP_EWORKSPACE;
    }
    if (!all_aligned16(x16, wi, wo, hd16, d_y, d_x, d_wi, d_wo, workspace)) {
        set_error("%s: x16, wi, wo, hd16, d_y, d_x, d_wi, d_wo and the workspace must be 16-byte aligned", who);
        return RQHIP_EARG;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool wgrad = d_wi || d_wo;
    __bf16 *dy16 = wgrad ? reinterpret_cast<__bf16 *>(workspace) : nullptr;
    __bf16 *g16 = d_wi ? reinterpret_cast<__bf16 *>(reinterpret_cast<char *>(workspace) + rqhip_t5_ffn_act_image_bytes(N, d)) : nullptr;
    {
        FfnRows a;      // d_wo alone: the kernel stages d_y, writes dy16 and returns
        a.x = d_y, a.w1 = wo, a.w2 = wi, a.h_in = reinterpret_cast<const float *>(hd16), a.mid = reinterpret_cast<float *>(g16);
        a.out = d_x, a.x16 = dy16, a.seed = nullptr, a.th = dropout_threshold(p), a.s = dropout_scale_f64(p);
        a.N = N, a.d = d, a.F = F;
        const int rc1 = ffn_rows<true, true, IMG, true>(a, s);
        if (rc1 != RQHIP_OK) return rc1;
    }
    if (wgrad) {
        FfnWgrad16 q;
        q.g = g16, q.x = reinterpret_cast<const __bf16 *>(x16), q.dy = dy16, q.h = reinterpret_cast<const __bf16 *>(hd16);
        q.d_wi = d_wi, q.d_wo = d_wo, q.N = N, q.d = d, q.F = F;
        const int tiles = (d / 32) * (F / 32);
        q.tiles_wi = d_wi ? tiles : 0;
        hipLaunchKernelGGL(t5_ffn_wgrad16_kernel, dim3((unsigned)(q.tiles_wi + (d_wo ? tiles : 0))), dim3(256), 0, s, q);
        RQ_CHECK_LAUNCH("t5_ffn_wgrad16_kernel");
    }
    return RQHIP_OK;
}

}  // namespace

extern "C" int rqhip_t5_ffn_fwd(const float *x, const float *wi, const float *wo, int64_t N, int d, int F, double p,
                                const int64_t *seed, float *y, float *h, rqhip_stream_t stream) {
    return ffn_fwd<false>("t5_ffn_fwd", x, wi, wo, N, d, F, p, seed, y, h, stream);
}

extern "C" int rqhip_t5_ffn_fwd_bf16(const float *x, const float *wi, const float *wo, int64_t N, int d, int F, double p,
                                     const int64_t *seed, float *y, float *h, rqhip_stream_t stream) {
    return ffn_fwd<true>("t5_ffn_fwd_bf16", x, wi, wo, N, d, F, p, seed, y, h, stream);
}

extern "C" int rqhip_t5_ffn_bwd(const float *x, const float *wi, const float *wo, const float *h, const float *d_y,
                                int64_t N, int d, int F, double p, const int64_t *seed, float *d_x, float *d_wi,
                                float *d_wo, void *workspace, rqhip_stream_t stream) {
    return ffn_bwd<false>("t5_ffn_bwd", x, wi, wo, h, d_y, N, d, F, p, seed, d_x, d_wi, d_wo, workspace, stream);
}

extern "C" int rqhip_t5_ffn_bwd_bf16(const float *x, const float *wi, const float *wo, const float *h, const float *d_y,
                                     int64_t N, int d, int F, double p, const int64_t *seed, float *d_x, float *d_wi,
                                     float *d_wo, void *workspace, rqhip_stream_t stream) {
    return ffn_bwd<true>("t5_ffn_bwd_bf16", x, wi, wo, h, d_y, N, d, F, p, seed, d_x, d_wi, d_wo, workspace, stream);
}

extern "C" int rqhip_t5_ffn_fwd_bf16w(const float *x, const rqhip_bf16_t *wi16, const rqhip_bf16_t *wo16, int64_t N, int d,
                                      int F, double p, const int64_t *seed, float *y, float *h, rqhip_stream_t stream) {
    return ffn_fwd<true, true>("t5_ffn_fwd_bf16w", x, reinterpret_cast<const float *>(wi16),
                               reinterpret_cast<const float *>(wo16), N, d, F, p, seed, y, h, stream);
}

extern "C" int rqhip_t5_ffn_bwd_bf16w(const float *x, const rqhip_bf16_t *wi16t, const rqhip_bf16_t *wo16t, const float *h,
                                      const float *d_y, int64_t N, int d, int F, double p, const int64_t *seed, float *d_x,
                                      float *d_wi, float *d_wo, void *workspace, rqhip_stream_t stream) {
    return ffn_bwd<true, true>("t5_ffn_bwd_bf16w", x, reinterpret_cast<const float *>(wi16t),
                               reinterpret_cast<const float *>(wo16t), h, d_y, N, d, F, p, seed, d_x, d_wi, d_wo, workspace,
                               stream);
}

extern "C" int rqhip_t5_ffn_fwd_bf16a(const float *x, const float *wi, const float *wo, int64_t N, int d, int F, double p,
                                      const int64_t *seed, float *y, rqhip_bf16_t *hd16, rqhip_bf16_t *x16,
                                      rqhip_stream_t stream) {
    return ffn_fwd<true, false, true>("t5_ffn_fwd_bf16a", x, wi, wo, N, d, F, p, seed, y, reinterpret_cast<float *>(hd16),
                                      stream, x16);
}

extern "C" int rqhip_t5_ffn_fwd_bf16wa(const float *x, const rqhip_bf16_t *wi16, const rqhip_bf16_t *wo16, int64_t N, int d,
                                       int F, double p, const int64_t *seed, float *y, rqhip_bf16_t *hd16, rqhip_bf16_t *x16,
                                       rqhip_stream_t stream) {
    return ffn_fwd<true, true, true>("t5_ffn_fwd_bf16wa", x, reinterpret_cast<const float *>(wi16),
                                     reinterpret_cast<const float *>(wo16), N, d, F, p, seed, y,
                                     reinterpret_cast<float *>(hd16), stream, x16);
}

extern "C" int rqhip_t5_ffn_bwd_bf16a(const rqhip_bf16_t *x16, const float *wi, const float *wo, const rqhip_bf16_t *hd16,
                                      const float *d_y, int64_t N, int d, int F, double p, float *d_x, float *d_wi,
                                      float *d_wo, void *workspace, rqhip_stream_t stream) {
    return ffn_bwd_act<false>("t5_ffn_bwd_bf16a", x16, wi, wo, hd16, d_y, N, d, F, p, d_x, d_wi, d_wo, workspace, stream);
}

extern "C" int rqhip_t5_ffn_bwd_bf16wa(const rqhip_bf16_t *x16, const rqhip_bf16_t *wi16t, const rqhip_bf16_t *wo16t,
                                       const rqhip_bf16_t *hd16, const float *d_y, int64_t N, int d, int F, double p,
                                       float *d_x, float *d_wi, float *d_wo, void *workspace, rqhip_stream_t stream) {
    return ffn_bwd_act<true>("t5_ffn_bwd_bf16wa", x16, reinterpret_cast<const float *>(wi16t),
                             reinterpret_cast<const float *>(wo16t), hd16, d_y, N, d, F, p, d_x, d_wi, d_wo, workspace, stream);
}

// t5_attention_long.hip -- the fused T5 attention of t5_attention.hip for sequences beyond its 256 tokens (gfx950):
// inference, the training forward and the backward, tiled over the keys with an online softmax.
//
// Same mathematics and T5 semantics as t5_attention.hip (fp32 on v_mfma_f32_16x16x4_f32, d_kv = 64, no 1/sqrt(d),
// finfo(float32).min ADDED to masked scores, rows read and written at their strides), and the same register layouts:
//   S^T = K Q^T   lane (g, i) ends with S[i][16 mt + 4 g + r] of the chunk's key tile mt,
//   O^T = V^T P^T the lane's own p registers are the B operand; lane (g, i) ends with O[i][16 dt + 4 g + 0..3].
// What differs: a workgroup never holds more than ONE chunk of kLongChunk keys (forward, query-major backward) or of
// kLongChunk queries (key-major backward) in LDS, at the 68-float row stride, and walks the chunks in ascending order.
//
// Forward, one workgroup per (K/V group, head, block of kLongQb query rows), a wave per sixteen rows.  Per chunk, in
// this order (m, l: the row's running max and sum; o: its unnormalised output; all start at -inf, 0, 0):
//   s_j     = q . k_j (+ bias) (+ -FLT_MAX when masked); -inf for a key at or beyond Tk
//   m'      = max(m, max_j s_j)            the lane's keys in (mt, r) order, then lanes xor 16, xor 32
//   alpha   = expf(m - m')                 0 on the first chunk, and when the row leaves a wholly masked prefix
//   p_j     = expf(s_j - m')
//   l       = l * alpha + sum_j p_j        EVERY p_j, dropped or not: the same order of lanes as the max
//   p_j     = 0 where the dropout decision drops (i, j)   (training only)
//   o       = o * alpha + V^T p            V^T p from zero, one MFMA per key, the chunk's keys ascending
//   m       = m'
// and behind the last chunk  out = o / l  (one IEEE divide), times 1.0f / (1.0f - (float)p) in the training forward;
// lse = m + logf(l), and the pair (m, l) beside it.  No chunk is skipped under `causal`: a row whose every key is
// masked weighs ALL Tk keys uniformly, the causally masked ones too, as with the operators.
//
// Backward: P_ij = expf(s_ij - m_i) / l_i from the saved pair, never from lse (which cannot carry log(l) beside
// m = -FLT_MAX).
//   t5_long_bwd_q_kernel  one workgroup per (row, head, slice of the query blocks), a wave per sixteen queries, the key
//     chunks walked TWICE: first D_i = sum_j P_ij dP_ij (dP = (dO V^T) o M / (1 - p); the lane's keys in chunk, mt, r
//     order, then lanes xor 16, xor 32), then dS = P o (dP - D), dQ^T += K^T dS^T and the sums of dS along the diagonals
//     j - i.  D comes from the very dP it is subtracted from, so a row with one live key has D = dP and dS = 0 exactly.
//     D goes to the workspace.  The diagonal sums: per tile through a per-wave 16 x 16 scratch into the wave's chunk-local
//     row, behind each chunk the four waves' rows in wave order into the workgroup's [Tq + Tk - 1] row, at the end that row
//     to the workspace.  A (row, head) has at most kLongBwdSlices such rows (slice s takes query blocks s, s + slices, ..),
//     so the workspace grows with Tq + Tk, not with Tq * Tk.
//   t5_long_bwd_kv_kernel  one workgroup per (row, head, block of kLongQb keys), a wave per sixteen keys (K and V rows
//     in registers), the queries walked in chunks of kLongChunk (Q, dO, m, l, D in LDS): dK^T += Q^T dS,
//     dV^T += dO^T (P o M / (1 - p)) in registers, queries ascending.
//   t5_long_dbias_reduce_kernel  adds the workspace rows of a head in (row, slice) ascending order.
// No float atomics, fixed orders everywhere: the same bits on every run, and a row's bits depend on Tq, Tk and that row's
// data only.  No allocation, copy, memset or sync; graph-capturable once a first eager call has raised the LDS attribute.
// Every kernel but the last exists in a second arithmetic, "bf16" (t5_long_*_bf16_kernel, behind the fp32 kernels): the
// same walk and the same fp32 softmax with bf16 operands on v_mfma_f32_16x16x32_bf16 and bf16 LDS images.
#include <float.h>
#include <math.h>

#include <initializer_list>

#include "rqhip_common.h"
#include "t5_common.h"

namespace rqhip {

namespace {

constexpr int kLongD = 64;          // d_kv
constexpr int kLongLd = 68;         // LDS row stride (floats), as in t5_attention.hip
constexpr int kLongMaxT = 2048;     // Tq, Tk
constexpr int kLongChunk = 128;     // keys (forward, bwd_q) or queries (bwd_kv) in LDS at a time: RQHIP_T5_ATTENTION_LONG_CHUNK
constexpr int kLongQb = 64;         // query rows (keys in bwd_kv) of a workgroup: RQHIP_T5_ATTENTION_LONG_QBLOCK
constexpr int kLongBwdSlices = 4;   // workgroups per (row, head) of the query-major backward, at most
constexpr int kLongTiles = kLongChunk / 16;
constexpr int kLongThreads = 4 * RQ_WAVE;
constexpr int kLongDiagW = kLongChunk + 16;  // a wave's chunk-local diagonal row: 143 diagonals, padded
constexpr int kLongTileLd = 17;              // row stride of the per-wave 16 x 16 dS scratch

static_assert(kLongQb == 16 * (kLongThreads / RQ_WAVE), "a wave takes sixteen rows of its workgroup's block");

struct LongArgs {
    const float *q, *k, *v;
    float *out;
    long long ld_q, ld_kv, ld_out;
    int beams, H, Tq, Tk, causal, nqb;
    const float *bias;  // [n_delta, H] or null
    int bias_base;      // table row of delta = -(Tq - 1)
    const unsigned char *key_mask;  // [Rk, Tk] or null
};

struct LongTrain {
    float *lse;             // [R, H, Tq]
    float *ml;              // [R, H, Tq, 2]: (m, l)
    const long long *seed;  // one int64 on the device (read only when thresh != 0)
    unsigned thresh;
    float inv_keep;
};

// rows [0, 16 * ntiles) of two LDS images from rows row0 .. of a [., lda] and a [., ldb] tensor; zeros at and beyond `rows`
__device__ __forceinline__ void long_stage_pair(float *As, float *Bs, const float *a, const float *b, size_t tok0, int row0,
                                                int rows, int ntiles, size_t lda, size_t ldb, size_t col) {
    for (int idx = threadIdx.x; idx < ntiles * 256; idx += blockDim.x) {
        const int j = idx >> 4, c = idx & 15;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
        if (row0 + j < rows) {
            const size_t row = tok0 + (size_t)(row0 + j);
            x = *reinterpret_cast<const float4 *>(a + row * lda + col + 4 * c);
            y = *reinterpret_cast<const float4 *>(b + row * ldb + col + 4 * c);
        }
        *reinterpret_cast<float4 *>(As + j * kLongLd + 4 * c) = x;
        *reinterpret_cast<float4 *>(Bs + j * kLongLd + 4 * c) = y;
    }
}

// 0: kept, -FLT_MAX: masked, -inf: at or beyond Tk -- for keys c0 .. c0 + 16 * ntiles - 1 of K/V group b
__device__ __forceinline__ void long_stage_madd(float *madd, const unsigned char *key_mask, long long b, int c0, int Tk,
                                                int ntiles) {
    for (int j = threadIdx.x; j < 16 * ntiles; j += blockDim.x) {
        const int key = c0 + j;
        madd[j] = key >= Tk ? -INFINITY : ((key_mask && !key_mask[b * Tk + key]) ? -FLT_MAX : 0.f);
    }
}

// One 16 x 16 tile of 64-term dot products, A rows in LDS (`ap`: the lane's row, + g), B in the lane's registers: FOUR
// independent chains of sixteen terms each (features 16 c .. 16 c + 15 in ascending order, from +0), added as
// (c0 + c1) + (c2 + c3).  Shorter chains round less than one chain of 64 (scores reach 40 and beyond, where one ulp is
// 4e-6 and the softmax turns an absolute score error into a relative weight error); every kernel of this file forms its
// scores and its dP with this one function, so the backward's s has the forward's bits.
__device__ __forceinline__ f32x4 long_dot64(const float *ap, const float (&b)[16]) {
    f32x4 c[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        c[x] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 4 * x; e < 4 * x + 4; ++e) c[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[4 * e], b[e], c[x], 0, 0, 0);
    }
    f32x4 r;
#pragma unroll
    for (int y = 0; y < 4; ++y) r[y] = (c[0][y] + c[1][y]) + (c[2][y] + c[3][y]);
    return r;
}

template <bool TRAIN>
__device__ __forceinline__ void long_fwd_body(LongArgs a, LongTrain t) {
    extern __shared__ float long_lds[];
    float *Ks = long_lds;
    float *Vs = Ks + kLongChunk * kLongLd;
    float *madd = Vs + kLongChunk * kLongLd;
    float *bias_s = madd + kLongChunk;  // [Tq + Tk - 1] of this head, by j - i + Tq - 1

    const int qb = blockIdx.x % a.nqb;
    const long long bh = blockIdx.x / a.nqb;
    const long long b = bh / a.H;
    const int h = (int)(bh - b * a.H);
    const int tid = threadIdx.x;
    const int wave = tid / RQ_WAVE, lane = tid & (RQ_WAVE - 1);
    const int i = lane & 15, g = lane >> 4;

    if (a.bias)
        for (int x = tid; x < a.Tq + a.Tk - 1; x += blockDim.x) bias_s[x] = a.bias[(size_t)(a.bias_base + x) * a.H + h];

    const int M = a.beams * a.Tq;
    const int m0 = qb * kLongQb + wave * 16;
    const bool active = m0 < M;  // wave-uniform
    const int m = m0 + i;
    const int mc = m < M ? m : M - 1;  // lanes past the last query recompute it and store nothing
    const int beam = mc / a.Tq, ti = mc - beam * a.Tq;
    const size_t qrow = (size_t)(b * a.beams + beam) * (size_t)a.Tq + (size_t)ti;
    const size_t qh = ((size_t)(b * a.beams + beam) * (size_t)a.H + (size_t)h) * (size_t)a.Tq + (size_t)ti;
    float qreg[16];
    if (active) {
        const float *qp = a.q + qrow * (size_t)a.ld_q + (size_t)h * kLongD + g;
#pragma unroll
        for (int e = 0; e < 16; ++e) qreg[e] = qp[4 * e];
    }
    unsigned long long seed = 0ull;
    if constexpr (TRAIN)
        if (t.thresh) seed = (unsigned long long)*t.seed;

    float run_m = -INFINITY, run_l = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int c0 = 0; c0 < a.Tk; c0 += kLongChunk) {
        const int nk = a.Tk - c0 < kLongChunk ? a.Tk - c0 : kLongChunk;
        const int ntiles = (nk + 15) >> 4;
        __syncthreads();  // the previous chunk's readers are done
        long_stage_pair(Ks, Vs, a.k, a.v, (size_t)b * (size_t)a.Tk, c0, a.Tk, ntiles, (size_t)a.ld_kv, (size_t)a.ld_kv,
                        (size_t)h * kLongD);
        long_stage_madd(madd, a.key_mask, b, c0, a.Tk, ntiles);
        __syncthreads();
        if (!active) continue;

        // ---- the chunk's scores, bias, masks and max
        f32x4 s[kLongTiles];
        float mx = -INFINITY;
#pragma unroll
        for (int mt = 0; mt < kLongTiles; ++mt) {
            s[mt] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (mt < ntiles) {
                const f32x4 acc = long_dot64(Ks + (16 * mt + i) * kLongLd + g, qreg);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int jl = 16 * mt + 4 * g + r, j = c0 + jl;
                    const float ma = madd[jl];
                    float sc = acc[r];
                    if (ma == -INFINITY) {
                        sc = -INFINITY;
                    } else {
                        if (a.bias) sc = sc + bias_s[j - ti + a.Tq - 1];
                        if (ma != 0.f || (a.causal && j > ti)) sc = sc + -FLT_MAX;
                    }
                    s[mt][r] = sc;
                    mx = fmaxf(mx, sc);
                }
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, RQ_WAVE));
        mx = fmaxf(mx, __shfl_xor(mx, 32, RQ_WAVE));
        const float m_new = fmaxf(run_m, mx);  // finite: a chunk holds at least one key below Tk
        const float alpha = expf(run_m - m_new);

        // ---- exp, the chunk's sum, the rescale
        float sum = 0.f;
#pragma unroll
        for (int mt = 0; mt < kLongTiles; ++mt) {
            if (mt < ntiles) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = expf(s[mt][r] - m_new);
                    s[mt][r] = p;
                    sum = sum + p;
                }
            }
        }
        sum = sum + __shfl_xor(sum, 16, RQ_WAVE);
        sum = sum + __shfl_xor(sum, 32, RQ_WAVE);
        run_l = run_l * alpha + sum;
        run_m = m_new;
        if constexpr (TRAIN) {
            if (t.thresh) {  // the dropped weights leave the product, the sum stays
#pragma unroll
                for (int mt = 0; mt < kLongTiles; ++mt) {
                    if (mt < ntiles) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (!dropout_keep(seed, (unsigned long long)qh * a.Tk + (c0 + 16 * mt + 4 * g + r), t.thresh))
                                s[mt][r] = 0.f;
                    }
                }
            }
        }

        // ---- the chunk's V^T P^T from zero, then O^T = O^T alpha + it
        f32x4 oc[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) oc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mt = 0; mt < kLongTiles; ++mt) {
            if (mt < ntiles) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float *vp = Vs + (16 * mt + 4 * g + r) * kLongLd + i;
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt)
                        oc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[16 * dt], s[mt][r], oc[dt], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[dt][r] = o[dt][r] * alpha + oc[dt][r];
    }

    if (active && m < M) {
        float *op = a.out + qrow * (size_t)a.ld_out + (size_t)h * kLongD + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            if constexpr (TRAIN)
                *reinterpret_cast<float4 *>(op + 16 * dt) =
                    make_float4(o[dt][0] / run_l * t.inv_keep, o[dt][1] / run_l * t.inv_keep,
                                o[dt][2] / run_l * t.inv_keep, o[dt][3] / run_l * t.inv_keep);
            else
                *reinterpret_cast<float4 *>(op + 16 * dt) =
                    make_float4(o[dt][0] / run_l, o[dt][1] / run_l, o[dt][2] / run_l, o[dt][3] / run_l);
        }
        if constexpr (TRAIN) {
            if (g == 0) {
                t.lse[qh] = run_m + logf(run_l);
                t.ml[2 * qh] = run_m;
                t.ml[2 * qh + 1] = run_l;
            }
        }
    }
}

__global__ __launch_bounds__(kLongThreads) void t5_long_fwd_kernel(LongArgs a) { long_fwd_body<false>(a, LongTrain{}); }

__global__ __launch_bounds__(kLongThreads) void t5_long_fwd_train_kernel(LongArgs a, LongTrain t) {
    long_fwd_body<true>(a, t);
}

// ---- backward

struct LongBwdArgs {
    const float *q, *k, *v, *d_out, *ml;
    float *dq, *dk, *dv, *dd, *dbias_part;  // dd [R, H, Tq] and dbias_part [R * H * nsb, Tq + Tk - 1]: the workspace
    long long ld_q, ld_kv, ld_do;
    int H, Tq, Tk, causal, nqb, nsb, nkb;
    const float *bias;
    int bias_base;
    const unsigned char *key_mask;
    const long long *seed;
    unsigned thresh;
    float inv_keep;
};

__global__ __launch_bounds__(kLongThreads) void t5_long_bwd_q_kernel(LongBwdArgs a) {
    extern __shared__ float long_lds[];
    const int nb = a.bias ? a.Tq + a.Tk - 1 : 0;
    float *Ks = long_lds;
    float *Vs = Ks + kLongChunk * kLongLd;
    float *madd = Vs + kLongChunk * kLongLd;
    float *dbw_all = madd + kLongChunk;                               // [4][kLongDiagW]
    float *tile_all = dbw_all + (kLongThreads / RQ_WAVE) * kLongDiagW;  // [4][16 * kLongTileLd]
    float *bias_s = tile_all + (kLongThreads / RQ_WAVE) * 16 * kLongTileLd;  // [nb]
    float *drow = bias_s + nb;                                        // [nb]: this workgroup's diagonal sums

    const int sb = blockIdx.x % a.nsb;
    const long long bh = blockIdx.x / a.nsb;
    const long long b = bh / a.H;
    const int h = (int)(bh - b * a.H);
    const int tid = threadIdx.x;
    const int wave = tid / RQ_WAVE, lane = tid & (RQ_WAVE - 1);
    const int i = lane & 15, g = lane >> 4;
    float *dbw = dbw_all + wave * kLongDiagW, *tile = tile_all + wave * 16 * kLongTileLd;
    const unsigned long long seed = a.thresh ? (unsigned long long)*a.seed : 0ull;

    for (int x = tid; x < nb; x += blockDim.x) {
        bias_s[x] = a.bias[(size_t)(a.bias_base + x) * a.H + h];
        drow[x] = 0.f;
    }

    for (int qb = sb; qb < a.nqb; qb += a.nsb) {
        const int q0 = qb * kLongQb, m0 = q0 + wave * 16;
        const bool active = m0 < a.Tq;  // wave-uniform
        const int m = m0 + i;
        const int ti = m < a.Tq ? m : a.Tq - 1;  // lanes past the last query recompute it and contribute nothing
        const size_t qrow = (size_t)b * (size_t)a.Tq + (size_t)ti;
        const size_t qh = ((size_t)b * (size_t)a.H + (size_t)h) * (size_t)a.Tq + (size_t)ti;
        float qreg[16], doreg[16], mx = 0.f, sum = 1.f;
        if (active) {
            const float *qp = a.q + qrow * (size_t)a.ld_q + (size_t)h * kLongD + g;
            const float *dop = a.d_out + qrow * (size_t)a.ld_do + (size_t)h * kLongD + g;
#pragma unroll
            for (int e = 0; e < 16; ++e) qreg[e] = qp[4 * e], doreg[e] = dop[4 * e];
            mx = a.ml[2 * qh], sum = a.ml[2 * qh + 1];
        }
        float D = 0.f;
        f32x4 dq[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int pass = 0; pass < 2; ++pass) {
            float Dl = 0.f;
            for (int c0 = 0; c0 < a.Tk; c0 += kLongChunk) {
                const int nk = a.Tk - c0 < kLongChunk ? a.Tk - c0 : kLongChunk;
                const int ntiles = (nk + 15) >> 4;
                __syncthreads();  // the previous chunk's readers (and the reduction of its diagonal rows) are done
                long_stage_pair(Ks, Vs, a.k, a.v, (size_t)b * (size_t)a.Tk, c0, a.Tk, ntiles, (size_t)a.ld_kv,
                                (size_t)a.ld_kv, (size_t)h * kLongD);
                long_stage_madd(madd, a.key_mask, b, c0, a.Tk, ntiles);
                const bool diag = pass == 1 && a.bias != nullptr;
                if (diag)
                    for (int x = lane; x < kLongDiagW; x += RQ_WAVE) dbw[x] = 0.f;  // the wave's own row
                __syncthreads();
                if (active) {
                    f32x4 dqc[4];  // the chunk's dS K from zero
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) dqc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    for (int mt = 0; mt < ntiles; ++mt) {
                        const f32x4 sacc = long_dot64(Ks + (16 * mt + i) * kLongLd + g, qreg);
                        const f32x4 pacc = long_dot64(Vs + (16 * mt + i) * kLongLd + g, doreg);
                        f32x4 ds;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int jl = 16 * mt + 4 * g + r, j = c0 + jl;
                            const float ma = madd[jl];
                            float sc = sacc[r];
                            if (ma == -INFINITY) {
                                sc = -INFINITY;
                            } else {
                                if (a.bias) sc = sc + bias_s[j - ti + a.Tq - 1];
                                if (ma != 0.f || (a.causal && j > ti)) sc = sc + -FLT_MAX;
                            }
                            const float p = expf(sc - mx) / sum;
                            float d = pacc[r];
                            if (a.thresh)
                                d = dropout_keep(seed, (unsigned long long)qh * a.Tk + j, a.thresh) ? d * a.inv_keep : 0.f;
                            Dl = Dl + p * d;
                            const float x = p * (d - D);
                            ds[r] = m < a.Tq ? x : 0.f;
                        }
                        if (pass == 1) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float *k2 = Ks + (16 * mt + 4 * g + r) * kLongLd + i;
#pragma unroll
                                for (int dt = 0; dt < 4; ++dt)
                                    dqc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(k2[16 * dt], ds[r], dqc[dt], 0, 0, 0);
                            }
                            if (diag) {
#pragma unroll
                                for (int r = 0; r < 4; ++r) tile[i * kLongTileLd + 4 * g + r] = ds[r];
                                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // scratch and row are this wave's only
                                if (lane < 31) {
                                    const int dl = lane - 15;  // key - query inside the tile
                                    const int lo = dl < 0 ? -dl : 0, hi = dl > 0 ? 15 - dl : 15;
                                    float acc1 = 0.f;
                                    for (int ii = lo; ii <= hi; ++ii) acc1 = acc1 + tile[ii * kLongTileLd + ii + dl];
                                    const int xl = 16 * mt + dl + 15;  // < 16 * 7 + 15 + 15 + 1 = kLongDiagW - 1
                                    dbw[xl] = dbw[xl] + acc1;
                                }
                                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                            }
                        }
                    }
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) dq[dt][r] = dq[dt][r] + dqc[dt][r];
                }
                if (diag) {  // the waves' rows in wave order into the workgroup's row
                    __syncthreads();
                    const int xg = tid;  // (key - c0) - (query - q0) + kLongQb - 1
                    if (xg < kLongChunk + kLongQb - 1) {
                        const int X = xg - (kLongQb - 1) + c0 - q0 + a.Tq - 1;
                        if (X >= 0 && X < nb) {
                            float acc1 = drow[X];
                            for (int w = 0; w < kLongThreads / RQ_WAVE; ++w) {
                                const int xl = xg - (kLongQb - 16) + 16 * w;
                                if (xl >= 0 && xl < kLongDiagW) acc1 = acc1 + dbw_all[w * kLongDiagW + xl];
                            }
                            drow[X] = acc1;
                        }
                    }
                }
            }
            if (pass == 0) {
                Dl = Dl + __shfl_xor(Dl, 16, RQ_WAVE);
                Dl = Dl + __shfl_xor(Dl, 32, RQ_WAVE);
                D = Dl;
                if (active && m < a.Tq && g == 0) a.dd[qh] = D;
            }
        }
        if (active && m < a.Tq) {
            float *dqp = a.dq + qrow * (size_t)a.H * kLongD + (size_t)h * kLongD + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<float4 *>(dqp + 16 * dt) = make_float4(dq[dt][0], dq[dt][1], dq[dt][2], dq[dt][3]);
        }
    }
    __syncthreads();
    for (int x = tid; x < nb; x += blockDim.x) a.dbias_part[(size_t)blockIdx.x * nb + x] = drow[x];
}

__global__ __launch_bounds__(kLongThreads) void t5_long_bwd_kv_kernel(LongBwdArgs a) {
    extern __shared__ float long_lds[];
    float *Qs = long_lds;
    float *dOs = Qs + kLongChunk * kLongLd;
    float *mx_s = dOs + kLongChunk * kLongLd;
    float *sum_s = mx_s + kLongChunk;
    float *dd_s = sum_s + kLongChunk;
    float *bias_s = dd_s + kLongChunk;  // [Tq + Tk - 1]

    const int kb = blockIdx.x % a.nkb;
    const long long bh = blockIdx.x / a.nkb;
    const long long b = bh / a.H;
    const int h = (int)(bh - b * a.H);
    const int tid = threadIdx.x;
    const int wave = tid / RQ_WAVE, lane = tid & (RQ_WAVE - 1);
    const int i = lane & 15, g = lane >> 4;
    const unsigned long long seed = a.thresh ? (unsigned long long)*a.seed : 0ull;
    const unsigned long long idx0 = ((unsigned long long)b * a.H + h) * (unsigned long long)a.Tq;  // + i, then * Tk + j

    if (a.bias)
        for (int x = tid; x < a.Tq + a.Tk - 1; x += blockDim.x) bias_s[x] = a.bias[(size_t)(a.bias_base + x) * a.H + h];

    const int j0 = kb * kLongQb + wave * 16;
    const bool active = j0 < a.Tk;  // wave-uniform
    const int j = j0 + i;
    const int jc = j < a.Tk ? j : a.Tk - 1;  // lanes past the last key recompute it and store nothing
    const size_t krow = (size_t)b * (size_t)a.Tk + (size_t)jc;
    float kreg[16], vreg[16], ma = 0.f;
    if (active) {
        const float *kp = a.k + krow * (size_t)a.ld_kv + (size_t)h * kLongD + g;
        const float *vp = a.v + krow * (size_t)a.ld_kv + (size_t)h * kLongD + g;
#pragma unroll
        for (int e = 0; e < 16; ++e) kreg[e] = kp[4 * e], vreg[e] = vp[4 * e];
        if (a.key_mask && !a.key_mask[b * a.Tk + jc]) ma = -FLT_MAX;
    }
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dk[dt] = dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int q0 = 0; q0 < a.Tq; q0 += kLongChunk) {
        const int nq = a.Tq - q0 < kLongChunk ? a.Tq - q0 : kLongChunk;
        const int ntiles = (nq + 15) >> 4;
        __syncthreads();
        long_stage_pair(Qs, dOs, a.q, a.d_out, (size_t)b * (size_t)a.Tq, q0, a.Tq, ntiles, (size_t)a.ld_q, (size_t)a.ld_do,
                        (size_t)h * kLongD);
        for (int x = tid; x < 16 * ntiles; x += blockDim.x) {
            const bool live = q0 + x < a.Tq;
            const size_t qh = (size_t)idx0 + (size_t)(live ? q0 + x : 0);
            mx_s[x] = live ? a.ml[2 * qh] : 0.f;
            sum_s[x] = live ? a.ml[2 * qh + 1] : 1.f;
            dd_s[x] = live ? a.dd[qh] : 0.f;
        }
        __syncthreads();
        if (!active) continue;
        f32x4 dkc[4], dvc[4];  // the chunk's sums from zero
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dkc[dt] = dvc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int qt = 0; qt < ntiles; ++qt) {
            const f32x4 sacc = long_dot64(Qs + (16 * qt + i) * kLongLd + g, kreg);
            const f32x4 pacc = long_dot64(dOs + (16 * qt + i) * kLongLd + g, vreg);
            f32x4 ds, pd;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ql = 16 * qt + 4 * g + r, qi = q0 + ql;
                const int ti = qi < a.Tq ? qi : a.Tq - 1;
                float sc = sacc[r];
                if (a.bias) sc = sc + bias_s[jc - ti + a.Tq - 1];
                if (ma != 0.f || (a.causal && j > ti)) sc = sc + -FLT_MAX;
                float p = expf(sc - mx_s[ql]) / sum_s[ql];
                if (qi >= a.Tq || j >= a.Tk) p = 0.f;
                float dp = pacc[r], pk = p;
                if (a.thresh) {
                    const bool keep = dropout_keep(seed, (idx0 + ti) * a.Tk + jc, a.thresh);
                    dp = keep ? dp * a.inv_keep : 0.f;
                    pk = keep ? p * a.inv_keep : 0.f;
                }
                ds[r] = p * (dp - dd_s[ql]);
                pd[r] = pk;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float *q2 = Qs + (16 * qt + 4 * g + r) * kLongLd + i, *do2 = dOs + (16 * qt + 4 * g + r) * kLongLd + i;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    dkc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(q2[16 * dt], ds[r], dkc[dt], 0, 0, 0);
                    dvc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(do2[16 * dt], pd[r], dvc[dt], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) dk[dt][r] = dk[dt][r] + dkc[dt][r], dv[dt][r] = dv[dt][r] + dvc[dt][r];
    }
    if (active && j < a.Tk) {
        const size_t off = krow * (size_t)a.H * kLongD + (size_t)h * kLongD + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            *reinterpret_cast<float4 *>(a.dk + off + 16 * dt) = make_float4(dk[dt][0], dk[dt][1], dk[dt][2], dk[dt][3]);
            *reinterpret_cast<float4 *>(a.dv + off + 16 * dt) = make_float4(dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]);
        }
    }
}

// ---- the "bf16" arithmetic of the four kernels above (contract: include/rqhip.h, rqhip_t5_attention_long_*_bf16).
// Storage, grids, chunk walk, softmax, dropout, D, dS and the diagonal sums are the fp32 arm's, in fp32 on unrounded
// values; only the operands of the matrix instructions are rounded to bf16 (nearest even), and every product is a chain
// of v_mfma_f32_16x16x32_bf16.  The register layouts are the fp32 arm's too (the C layout does not depend on the type).
//
// ONE assignment of reduction terms to the instruction's k-slots serves every product of the file: slot (g, e) of group
// s -- element e = 0 .. 7 of the A / B fragment of lane (g, .) -- is term 32 s + 16 (e >> 2) + 4 g + (e & 3).  That is
//   - for a lane's C registers, tiles 2 s and 2 s + 1 of its chunk (rows 16 (2 s) + 4 g + r and 16 (2 s + 1) + 4 g + r):
//     the eight p (dS, P o M) values it holds ARE its B fragment of group s, no lane movement;
//   - for an LDS image, two 8-byte reads at terms 32 s + 4 g and 32 s + 16 + 4 g of the lane's row, from a
//     [row][feature] image (stride kLongLdR; scores and dP, the features are the terms) or from a [feature][row] image
//     (stride kLongLdT; the products that sum over keys or queries).  The compiler joins the two into one ds_read2_b64,
//     which is served sixteen lanes (one g, sixteen rows) at a time over 32 banks: both strides are 2 * odd dwords, so
//     the sixteen 8-byte pieces cover the 32 banks once.
// The order of the terms inside a group is the instruction's; both operands use the same assignment, so each product
// meets its partner.  With an odd number of tiles the last half group multiplies zeros: the images are staged in whole
// groups of 32 rows, rows at and beyond the tensor's end as zeros, and the missing tile's weights are +0.

constexpr int kLongLdR = kLongD + 4;      // bf16 row stride of a [row][feature] image: 34 dwords
constexpr int kLongLdT = kLongChunk + 4;  // bf16 row stride of a [feature][row] image: 66 dwords
constexpr int kLongImgR = kLongChunk * kLongLdR;  // elements of the two images
constexpr int kLongImgT = kLongD * kLongLdT;

static_assert(kLongLdR % 8 == 4 && kLongLdT % 8 == 4, "row strides of 2 * odd dwords: 8-byte aligned rows");
static_assert(kLongImgR % 8 == 0 && kLongImgT % 8 == 0, "the images keep what follows them 16-byte aligned");

__device__ __forceinline__ bf16x8 long_frag_lds(const __bf16 *row, int g, int s) {
    const bf16x4 lo = *reinterpret_cast<const bf16x4 *>(row + 32 * s + 4 * g);
    const bf16x4 hi = *reinterpret_cast<const bf16x4 *>(row + 32 * s + 16 + 4 * g);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// the same fragment of a 64-float row in global memory (16-byte aligned), rounded as it is packed
__device__ __forceinline__ bf16x8 long_frag_global(const float *row, int g, int s) {
    const float4 lo = *reinterpret_cast<const float4 *>(row + 32 * s + 4 * g);
    const float4 hi = *reinterpret_cast<const float4 *>(row + 32 * s + 16 + 4 * g);
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return pack_bf16x8(v);
}

// Rows row0 .. row0 + nst - 1 (nst a multiple of 32) of a [., lda] tensor, rounded to bf16, as a [row][feature] image (RM)
// and / or a [feature][row] image (TR); zeros at and beyond `rows`.  A thread takes four rows by four features.
template <bool RM, bool TR>
__device__ __forceinline__ void long_stage_bf16(__bf16 *rm, __bf16 *tr, const float *a, size_t tok0, int row0, int rows,
                                                int nst, size_t lda, size_t col) {
    for (int idx = threadIdx.x; idx < nst * 4; idx += blockDim.x) {
        const int c = idx & 15, kq = idx >> 4;
        float x[4][4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row0 + 4 * kq + kk < rows)
                y = *reinterpret_cast<const float4 *>(a + (tok0 + (size_t)(row0 + 4 * kq + kk)) * lda + col + 4 * c);
            x[kk][0] = y.x, x[kk][1] = y.y, x[kk][2] = y.z, x[kk][3] = y.w;
        }
        if constexpr (RM) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                *reinterpret_cast<bf16x4 *>(rm + (4 * kq + kk) * kLongLdR + 4 * c) =
                    bf16x4{(__bf16)x[kk][0], (__bf16)x[kk][1], (__bf16)x[kk][2], (__bf16)x[kk][3]};
        }
        if constexpr (TR) {
#pragma unroll
            for (int f = 0; f < 4; ++f)
                *reinterpret_cast<bf16x4 *>(tr + (4 * c + f) * kLongLdT + 4 * kq) =
                    bf16x4{(__bf16)x[0][f], (__bf16)x[1][f], (__bf16)x[2][f], (__bf16)x[3][f]};
        }
    }
}

// long_dot64's twin: one 16 x 16 tile of 64-term dot products as ONE chain of two groups from +0, A rows in a
// [row][feature] image (`arow`: the lane's row), B in the lane's two fragments.  Every bf16 kernel forms its scores and
// its dP with this one function, so the backward's s has the forward's bits.
__device__ __forceinline__ f32x4 long_dot64_bf16(const __bf16 *arow, int g, const bf16x8 (&b)[2]) {
    f32x4 c = mma_group_bf16(long_frag_lds(arow, g, 0), b[0], f32x4{0.f, 0.f, 0.f, 0.f});
    return mma_group_bf16(long_frag_lds(arow, g, 1), b[1], c);
}

// whole groups of 32 that cover n rows
__device__ __forceinline__ int long_groups32(int n) { return ((n + 31) >> 5) << 5; }

template <bool TRAIN>
__device__ __forceinline__ void long_fwd_body_bf16(LongArgs a, LongTrain t) {
    extern __shared__ float long_lds[];
    __bf16 *Kb = reinterpret_cast<__bf16 *>(long_lds);  // [key][feature]
    __bf16 *Vt = Kb + kLongImgR;                        // [feature][key]
    float *madd = reinterpret_cast<float *>(Vt + kLongImgT);
    float *bias_s = madd + kLongChunk;  // [Tq + Tk - 1] of this head, by j - i + Tq - 1

    const int qb = blockIdx.x % a.nqb;
    const long long bh = blockIdx.x / a.nqb;
    const long long b = bh / a.H;
    const int h = (int)(bh - b * a.H);
    const int tid = threadIdx.x;
    const int wave = tid / RQ_WAVE, lane = tid & (RQ_WAVE - 1);
    const int i = lane & 15, g = lane >> 4;

    if (a.bias)
        for (int x = tid; x < a.Tq + a.Tk - 1; x += blockDim.x) bias_s[x] = a.bias[(size_t)(a.bias_base + x) * a.H + h];

    const int M = a.beams * a.Tq;
    const int m0 = qb * kLongQb + wave * 16;
    const bool active = m0 < M;  // wave-uniform
    const int m = m0 + i;
    const int mc = m < M ? m : M - 1;  // lanes past the last query recompute it and store nothing
    const int beam = mc / a.Tq, ti = mc - beam * a.Tq;
    const size_t qrow = (size_t)(b * a.beams + beam) * (size_t)a.Tq + (size_t)ti;
    const size_t qh = ((size_t)(b * a.beams + beam) * (size_t)a.H + (size_t)h) * (size_t)a.Tq + (size_t)ti;
    bf16x8 qf[2];
    if (active) {
        const float *qp = a.q + qrow * (size_t)a.ld_q + (size_t)h * kLongD;
        qf[0] = long_frag_global(qp, g, 0), qf[1] = long_frag_global(qp, g, 1);
    }
    unsigned long long seed = 0ull;
    if constexpr (TRAIN)
        if (t.thresh) seed = (unsigned long long)*t.seed;

    float run_m = -INFINITY, run_l = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int c0 = 0; c0 < a.Tk; c0 += kLongChunk) {
        const int nk = a.Tk - c0 < kLongChunk ? a.Tk - c0 : kLongChunk;
        const int ntiles = (nk + 15) >> 4;
        __syncthreads();  // the previous chunk's readers are done
        long_stage_bf16<true, false>(Kb, nullptr, a.k, (size_t)b * (size_t)a.Tk, c0, a.Tk, long_groups32(nk),
                                     (size_t)a.ld_kv, (size_t)h * kLongD);
        long_stage_bf16<false, true>(nullptr, Vt, a.v, (size_t)b * (size_t)a.Tk, c0, a.Tk, long_groups32(nk),
                                     (size_t)a.ld_kv, (size_t)h * kLongD);
        long_stage_madd(madd, a.key_mask, b, c0, a.Tk, ntiles);
        __syncthreads();
        if (!active) continue;

        // ---- the chunk's scores, bias, masks and max
        f32x4 s[kLongTiles];
        float mx = -INFINITY;
#pragma unroll
        for (int mt = 0; mt < kLongTiles; ++mt) {
            s[mt] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (mt < ntiles) {
                const f32x4 acc = long_dot64_bf16(Kb + (16 * mt + i) * kLongLdR, g, qf);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int jl = 16 * mt + 4 * g + r, j = c0 + jl;
                    const float ma = madd[jl];
                    float sc = acc[r];
                    if (ma == -INFINITY) {
                        sc = -INFINITY;
                    } else {
                        if (a.bias) sc = sc + bias_s[j - ti + a.Tq - 1];
                        if (ma != 0.f || (a.causal && j > ti)) sc = sc + -FLT_MAX;
                    }
                    s[mt][r] = sc;
                    mx = fmaxf(mx, sc);
                }
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, RQ_WAVE));
        mx = fmaxf(mx, __shfl_xor(mx, 32, RQ_WAVE));
        const float m_new = fmaxf(run_m, mx);  // finite: a chunk holds at least one key below Tk
        const float alpha = expf(run_m - m_new);

        // ---- exp, the chunk's sum (unrounded weights), the rescale
        float sum = 0.f;
#pragma unroll
        for (int mt = 0; mt < kLongTiles; ++mt) {
            if (mt < ntiles) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = expf(s[mt][r] - m_new);
                    s[mt][r] = p;
                    sum = sum + p;
                }
            }
        }
        sum = sum + __shfl_xor(sum, 16, RQ_WAVE);
        sum = sum + __shfl_xor(sum, 32, RQ_WAVE);
        run_l = run_l * alpha + sum;
        run_m = m_new;
        if constexpr (TRAIN) {
            if (t.thresh) {  // the dropped weights leave the product, the sum stays
#pragma unroll
                for (int mt = 0; mt < kLongTiles; ++mt) {
                    if (mt < ntiles) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (!dropout_keep(seed, (unsigned long long)qh * a.Tk + (c0 + 16 * mt + 4 * g + r), t.thresh))
                                s[mt][r] = 0.f;
                    }
                }
            }
        }

        // ---- the chunk's V^T P^T from zero, one instruction per 32 keys and 16 features, then O^T = O^T alpha + it
        f32x4 oc[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) oc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kg = 0; kg < kLongTiles / 2; ++kg) {
            if (2 * kg < ntiles) {
                float pv[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) pv[r] = s[2 * kg][r], pv[4 + r] = 2 * kg + 1 < ntiles ? s[2 * kg + 1][r] : 0.f;
                const bf16x8 pb = pack_bf16x8(pv);  // rounded after the dropout zeroing
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    oc[dt] = mma_group_bf16(long_frag_lds(Vt + (16 * dt + i) * kLongLdT, g, kg), pb, oc[dt]);
            }
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[dt][r] = o[dt][r] * alpha + oc[dt][r];
    }

    if (active && m < M) {
        float *op = a.out + qrow * (size_t)a.ld_out + (size_t)h * kLongD + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            if constexpr (TRAIN)
                *reinterpret_cast<float4 *>(op + 16 * dt) =
                    make_float4(o[dt][0] / run_l * t.inv_keep, o[dt][1] / run_l * t.inv_keep,
                                o[dt][2] / run_l * t.inv_keep, o[dt][3] / run_l * t.inv_keep);
            else
                *reinterpret_cast<float4 *>(op + 16 * dt) =
                    make_float4(o[dt][0] / run_l, o[dt][1] / run_l, o[dt][2] / run_l, o[dt][3] / run_l);
        }
        if constexpr (TRAIN) {
            if (g == 0) {
                t.lse[qh] = run_m + logf(run_l);
                t.ml[2 * qh] = run_m;
                t.ml[2 * qh + 1] = run_l;
            }
        }
    }
}

__global__ __launch_bounds__(kLongThreads) void t5_long_fwd_bf16_kernel(LongArgs a) {
    long_fwd_body_bf16<false>(a, LongTrain{});
}

__global__ __launch_bounds__(kLongThreads) void t5_long_fwd_train_bf16_kernel(LongArgs a, LongTrain t) {
    long_fwd_body_bf16<true>(a, t);
}

__global__ __launch_bounds__(kLongThreads) void t5_long_bwd_q_bf16_kernel(LongBwdArgs a) {
    extern __shared__ float long_lds[];
    const int nb = a.bias ? a.Tq + a.Tk - 1 : 0;
    __bf16 *Kb = reinterpret_cast<__bf16 *>(long_lds);  // [key][feature]: the scores
    __bf16 *Vb = Kb + kLongImgR;                        // [key][feature]: dP
    __bf16 *Kt = Vb + kLongImgR;                        // [feature][key]: dQ (second pass only)
    float *madd = reinterpret_cast<float *>(Kt + kLongImgT);
    float *dbw_all = madd + kLongChunk;                               // [4][kLongDiagW]
    float *tile_all = dbw_all + (kLongThreads / RQ_WAVE) * kLongDiagW;  // [4][16 * kLongTileLd]
    float *bias_s = tile_all + (kLongThreads / RQ_WAVE) * 16 * kLongTileLd;  // [nb]
    float *drow = bias_s + nb;                                        // [nb]: this workgroup's diagonal sums

    const int sb = blockIdx.x % a.nsb;
    const long long bh = blockIdx.x / a.nsb;
    const long long b = bh / a.H;
    const int h = (int)(bh - b * a.H);
    const int tid = threadIdx.x;
    const int wave = tid / RQ_WAVE, lane = tid & (RQ_WAVE - 1);
    const int i = lane & 15, g = lane >> 4;
    float *dbw = dbw_all + wave * kLongDiagW, *tile = tile_all + wave * 16 * kLongTileLd;
    const unsigned long long seed = a.thresh ? (unsigned long long)*a.seed : 0ull;

    for (int x = tid; x < nb; x += blockDim.x) {
        bias_s[x] = a.bias[(size_t)(a.bias_base + x) * a.H + h];
        drow[x] = 0.f;
    }

    for (int qb = sb; qb < a.nqb; qb += a.nsb) {
        const int q0 = qb * kLongQb, m0 = q0 + wave * 16;
        const bool active = m0 < a.Tq;  // wave-uniform
        const int m = m0 + i;
        const int ti = m < a.Tq ? m : a.Tq - 1;  // lanes past the last query recompute it and contribute nothing
        const size_t qrow = (size_t)b * (size_t)a.Tq + (size_t)ti;
        const size_t qh = ((size_t)b * (size_t)a.H + (size_t)h) * (size_t)a.Tq + (size_t)ti;
        bf16x8 qf[2], dof[2];
        float mx = 0.f, sum = 1.f;
        if (active) {
            const float *qp = a.q + qrow * (size_t)a.ld_q + (size_t)h * kLongD;
            const float *dop = a.d_out + qrow * (size_t)a.ld_do + (size_t)h * kLongD;
            qf[0] = long_frag_global(qp, g, 0), qf[1] = long_frag_global(qp, g, 1);
            dof[0] = long_frag_global(dop, g, 0), dof[1] = long_frag_global(dop, g, 1);
            mx = a.ml[2 * qh], sum = a.ml[2 * qh + 1];
        }
        float D = 0.f;
        f32x4 dq[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int pass = 0; pass < 2; ++pass) {
            float Dl = 0.f;
            for (int c0 = 0; c0 < a.Tk; c0 += kLongChunk) {
                const int nk = a.Tk - c0 < kLongChunk ? a.Tk - c0 : kLongChunk;
                const int ntiles = (nk + 15) >> 4;
                __syncthreads();  // the previous chunk's readers (and the reduction of its diagonal rows) are done
                if (pass == 1)
                    long_stage_bf16<true, true>(Kb, Kt, a.k, (size_t)b * (size_t)a.Tk, c0, a.Tk, long_groups32(nk),
                                                (size_t)a.ld_kv, (size_t)h * kLongD);
                else
                    long_stage_bf16<true, false>(Kb, nullptr, a.k, (size_t)b * (size_t)a.Tk, c0, a.Tk, long_groups32(nk),
                                                 (size_t)a.ld_kv, (size_t)h * kLongD);
                long_stage_bf16<true, false>(Vb, nullptr, a.v, (size_t)b * (size_t)a.Tk, c0, a.Tk, long_groups32(nk),
                                             (size_t)a.ld_kv, (size_t)h * kLongD);
                long_stage_madd(madd, a.key_mask, b, c0, a.Tk, ntiles);
                const bool diag = pass == 1 && a.bias != nullptr;
                if (diag)
                    for (int x = lane; x < kLongDiagW; x += RQ_WAVE) dbw[x] = 0.f;  // the wave's own row
                __syncthreads();
                if (active) {
                    f32x4 dqc[4];  // the chunk's dS K from zero
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) dqc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    for (int kg = 0; 2 * kg < ntiles; ++kg) {
                        float dsv[8];  // dS of key tiles 2 kg and 2 kg + 1: the B fragment of the group
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const int mt = 2 * kg + u;
                            if (mt < ntiles) {  // wave-uniform
                                const f32x4 sacc = long_dot64_bf16(Kb + (16 * mt + i) * kLongLdR, g, qf);
                                const f32x4 pacc = long_dot64_bf16(Vb + (16 * mt + i) * kLongLdR, g, dof);
                                f32x4 ds;
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const int jl = 16 * mt + 4 * g + r, j = c0 + jl;
                                    const float ma = madd[jl];
                                    float sc = sacc[r];
                                    if (ma == -INFINITY) {
                                        sc = -INFINITY;
                                    } else {
                                        if (a.bias) sc = sc + bias_s[j - ti + a.Tq - 1];
                                        if (ma != 0.f || (a.causal && j > ti)) sc = sc + -FLT_MAX;
                                    }
                                    const float p = expf(sc - mx) / sum;
                                    float d = pacc[r];
                                    if (a.thresh)
                                        d = dropout_keep(seed, (unsigned long long)qh * a.Tk + j, a.thresh) ? d * a.inv_keep
                                                                                                              : 0.f;
                                    Dl = Dl + p * d;
                                    const float x = p * (d - D);
                                    ds[r] = m < a.Tq ? x : 0.f;
                                    dsv[4 * u + r] = ds[r];
                                }
                                if (diag) {  // the unrounded dS
#pragma unroll
                                    for (int r = 0; r < 4; ++r) tile[i * kLongTileLd + 4 * g + r] = ds[r];
                                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // scratch and row are this wave's only
                                    if (lane < 31) {
                                        const int dl = lane - 15;  // key - query inside the tile
                                        const int lo = dl < 0 ? -dl : 0, hi = dl > 0 ? 15 - dl : 15;
                                        float acc1 = 0.f;
                                        for (int ii = lo; ii <= hi; ++ii) acc1 = acc1 + tile[ii * kLongTileLd + ii + dl];
                                        const int xl = 16 * mt + dl + 15;  // < 16 * 7 + 15 + 15 + 1 = kLongDiagW - 1
                                        dbw[xl] = dbw[xl] + acc1;
                                    }
                                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                                }
                            } else {
#pragma unroll
                                for (int r = 0; r < 4; ++r) dsv[4 * u + r] = 0.f;
                            }
                        }
                        if (pass == 1) {
                            const bf16x8 dsb = pack_bf16x8(dsv);
#pragma unroll
                            for (int dt = 0; dt < 4; ++dt)
                                dqc[dt] = mma_group_bf16(long_frag_lds(Kt + (16 * dt + i) * kLongLdT, g, kg), dsb, dqc[dt]);
                        }
                    }
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) dq[dt][r] = dq[dt][r] + dqc[dt][r];
                }
                if (diag) {  // the waves' rows in wave order into the workgroup's row
                    __syncthreads();
                    const int xg = tid;  // (key - c0) - (query - q0) + kLongQb - 1
                    if (xg < kLongChunk + kLongQb - 1) {
                        const int X = xg - (kLongQb - 1) + c0 - q0 + a.Tq - 1;
                        if (X >= 0 && X < nb) {
                            float acc1 = drow[X];
                            for (int w = 0; w < kLongThreads / RQ_WAVE; ++w) {
                                const int xl = xg - (kLongQb - 16) + 16 * w;
                                if (xl >= 0 && xl < kLongDiagW) acc1 = acc1 + dbw_all[w * kLongDiagW + xl];
                            }
                            drow[X] = acc1;
                        }
                    }
                }
            }
            if (pass == 0) {
                Dl = Dl + __shfl_xor(Dl, 16, RQ_WAVE);
                Dl = Dl + __shfl_xor(Dl, 32, RQ_WAVE);
                D = Dl;
                if (active && m < a.Tq && g == 0) a.dd[qh] = D;
            }
        }
        if (active && m < a.Tq) {
            float *dqp = a.dq + qrow * (size_t)a.H * kLongD + (size_t)h * kLongD + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<float4 *>(dqp + 16 * dt) = make_float4(dq[dt][0], dq[dt][1], dq[dt][2], dq[dt][3]);
        }
    }
    __syncthreads();
    for (int x = tid; x < nb; x += blockDim.x) a.dbias_part[(size_t)blockIdx.x * nb + x] = drow[x];
}

__global__ __launch_bounds__(kLongThreads) void t5_long_bwd_kv_bf16_kernel(LongBwdArgs a) {
    extern __shared__ float long_lds[];
    __bf16 *Qb = reinterpret_cast<__bf16 *>(long_lds);  // [query][feature]: the scores
    __bf16 *dOb = Qb + kLongImgR;                       // [query][feature]: dP
    __bf16 *Qt = dOb + kLongImgR;                       // [feature][query]: dK
    __bf16 *dOt = Qt + kLongImgT;                       // [feature][query]: dV
    float *mx_s = reinterpret_cast<float *>(dOt + kLongImgT);
    float *sum_s = mx_s + kLongChunk;
    float *dd_s = sum_s + kLongChunk;
    float *bias_s = dd_s + kLongChunk;  // [Tq + Tk - 1]

    const int kb = blockIdx.x % a.nkb;
    const long long bh = blockIdx.x / a.nkb;
    const long long b = bh / a.H;
    const int h = (int)(bh - b * a.H);
    const int tid = threadIdx.x;
    const int wave = tid / RQ_WAVE, lane = tid & (RQ_WAVE - 1);
    const int i = lane & 15, g = lane >> 4;
    const unsigned long long seed = a.thresh ? (unsigned long long)*a.seed : 0ull;
    const unsigned long long idx0 = ((unsigned long long)b * a.H + h) * (unsigned long long)a.Tq;  // + i, then * Tk + j

    if (a.bias)
        for (int x = tid; x < a.Tq + a.Tk - 1; x += blockDim.x) bias_s[x] = a.bias[(size_t)(a.bias_base + x) * a.H + h];

    const int j0 = kb * kLongQb + wave * 16;
    const bool active = j0 < a.Tk;  // wave-uniform
    const int j = j0 + i;
    const int jc = j < a.Tk ? j : a.Tk - 1;  // lanes past the last key recompute it and store nothing
    const size_t krow = (size_t)b * (size_t)a.Tk + (size_t)jc;
    bf16x8 kf[2], vf[2];
    float ma = 0.f;
    if (active) {
        const float *kp = a.k + krow * (size_t)a.ld_kv + (size_t)h * kLongD;
        const float *vp = a.v + krow * (size_t)a.ld_kv + (size_t)h * kLongD;
        kf[0] = long_frag_global(kp, g, 0), kf[1] = long_frag_global(kp, g, 1);
        vf[0] = long_frag_global(vp, g, 0), vf[1] = long_frag_global(vp, g, 1);
        if (a.key_mask && !a.key_mask[b * a.Tk + jc]) ma = -FLT_MAX;
    }
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dk[dt] = dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int q0 = 0; q0 < a.Tq; q0 += kLongChunk) {
        const int nq = a.Tq - q0 < kLongChunk ? a.Tq - q0 : kLongChunk;
        const int ntiles = (nq + 15) >> 4;
        __syncthreads();
        long_stage_bf16<true, true>(Qb, Qt, a.q, (size_t)b * (size_t)a.Tq, q0, a.Tq, long_groups32(nq), (size_t)a.ld_q,
                                    (size_t)h * kLongD);
        long_stage_bf16<true, true>(dOb, dOt, a.d_out, (size_t)b * (size_t)a.Tq, q0, a.Tq, long_groups32(nq),
                                    (size_t)a.ld_do, (size_t)h * kLongD);
        for (int x = tid; x < 16 * ntiles; x += blockDim.x) {
            const bool live = q0 + x < a.Tq;
            const size_t qh = (size_t)idx0 + (size_t)(live ? q0 + x : 0);
            mx_s[x] = live ? a.ml[2 * qh] : 0.f;
            sum_s[x] = live ? a.ml[2 * qh + 1] : 1.f;
            dd_s[x] = live ? a.dd[qh] : 0.f;
        }
        __syncthreads();
        if (!active) continue;
        f32x4 dkc[4], dvc[4];  // the chunk's sums from zero
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dkc[dt] = dvc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int qg = 0; 2 * qg < ntiles; ++qg) {
            float dsv[8], pdv[8];  // dS and the dropped, scaled P of query tiles 2 qg and 2 qg + 1: the B fragments
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int qt = 2 * qg + u;
                if (qt < ntiles) {  // wave-uniform
                    const f32x4 sacc = long_dot64_bf16(Qb + (16 * qt + i) * kLongLdR, g, kf);
                    const f32x4 pacc = long_dot64_bf16(dOb + (16 * qt + i) * kLongLdR, g, vf);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ql = 16 * qt + 4 * g + r, qi = q0 + ql;
                        const int ti = qi < a.Tq ? qi : a.Tq - 1;
                        float sc = sacc[r];
                        if (a.bias) sc = sc + bias_s[jc - ti + a.Tq - 1];
                        if (ma != 0.f || (a.causal && j > ti)) sc = sc + -FLT_MAX;
                        float p = expf(sc - mx_s[ql]) / sum_s[ql];
                        if (qi >= a.Tq || j >= a.Tk) p = 0.f;
                        float dp = pacc[r], pk = p;
                        if (a.thresh) {
                            const bool keep = dropout_keep(seed, (idx0 + ti) * a.Tk + jc, a.thresh);
                            dp = keep ? dp * a.inv_keep : 0.f;
                            pk = keep ? p * a.inv_keep : 0.f;
                        }
                        dsv[4 * u + r] = p * (dp - dd_s[ql]);
                        pdv[4 * u + r] = pk;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) dsv[4 * u + r] = pdv[4 * u + r] = 0.f;
                }
            }
            const bf16x8 dsb = pack_bf16x8(dsv), pdb = pack_bf16x8(pdv);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                dkc[dt] = mma_group_bf16(long_frag_lds(Qt + (16 * dt + i) * kLongLdT, g, qg), dsb, dkc[dt]);
                dvc[dt] = mma_group_bf16(long_frag_lds(dOt + (16 * dt + i) * kLongLdT, g, qg), pdb, dvc[dt]);
            }
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) dk[dt][r] = dk[dt][r] + dkc[dt][r], dv[dt][r] = dv[dt][r] + dvc[dt][r];
    }
    if (active && j < a.Tk) {
        const size_t off = krow * (size_t)a.H * kLongD + (size_t)h * kLongD + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            *reinterpret_cast<float4 *>(a.dk + off + 16 * dt) = make_float4(dk[dt][0], dk[dt][1], dk[dt][2], dk[dt][3]);
            *reinterpret_cast<float4 *>(a.dv + off + 16 * dt) = make_float4(dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]);
        }
    }
}

// d_bias[row, h] = sum over the rows r, then the slices s, ascending, of part[((r * H + h) * nsb + s)][row - base]; zero
// outside the call's delta range.
__global__ __launch_bounds__(256) void t5_long_dbias_reduce_kernel(const float *part, long long R, int H, int nsb, int nb,
                                                                   int base, int n_delta, float *out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n_delta * H) return;
    const int row = (int)(idx / H), h = (int)(idx - (long long)row * H);
    float acc = 0.f;
    if (row >= base && row < base + nb)
        for (long long r = 0; r < R; ++r)
            for (int s = 0; s < nsb; ++s)
                acc = acc + part[(((size_t)r * H + h) * (size_t)nsb + s) * (size_t)nb + (row - base)];
    out[idx] = acc;
}

// ---- host side

bool long_supported(int d_kv, int H, int Tq, int Tk) {
    return d_kv == kLongD && H >= 1 && Tq >= 1 && Tq <= kLongMaxT && Tk >= 1 && Tk <= kLongMaxT;
}

size_t long_fwd_lds_bytes(int Tq, int Tk, bool bias) {
    return (size_t)(2 * kLongChunk * kLongLd + kLongChunk + (bias ? Tq + Tk - 1 : 0)) * sizeof(float);
}

size_t long_bwd_q_lds_bytes(int Tq, int Tk, bool bias) {
    return (size_t)(2 * kLongChunk * kLongLd + kLongChunk + (kLongThreads / RQ_WAVE) * (kLongDiagW + 16 * kLongTileLd) +
                    (bias ? 2 * (Tq + Tk - 1) : 0)) * sizeof(float);
}

size_t long_bwd_kv_lds_bytes(int Tq, int Tk, bool bias) {
    return (size_t)(2 * kLongChunk * kLongLd + 3 * kLongChunk + (bias ? Tq + Tk - 1 : 0)) * sizeof(float);
}

// the bf16 arm: bf16 images ([row][feature] kLongImgR, [feature][row] kLongImgT elements), the rest as above
size_t long_fwd_lds_bytes_bf16(int Tq, int Tk, bool bias) {
    return (size_t)(kLongImgR + kLongImgT) * sizeof(__bf16) + (size_t)(kLongChunk + (bias ? Tq + Tk - 1 : 0)) * sizeof(float);
}

size_t long_bwd_q_lds_bytes_bf16(int Tq, int Tk, bool bias) {
    return (size_t)(2 * kLongImgR + kLongImgT) * sizeof(__bf16) +
           (size_t)(kLongChunk + (kLongThreads / RQ_WAVE) * (kLongDiagW + 16 * kLongTileLd) +
                    (bias ? 2 * (Tq + Tk - 1) : 0)) * sizeof(float);
}

size_t long_bwd_kv_lds_bytes_bf16(int Tq, int Tk, bool bias) {
    return (size_t)(2 * kLongImgR + 2 * kLongImgT) * sizeof(__bf16) +
           (size_t)(3 * kLongChunk + (bias ? Tq + Tk - 1 : 0)) * sizeof(float);
}

int long_blocks(int rows) { return (rows + kLongQb - 1) / kLongQb; }

int long_slices(int Tq) { return long_blocks(Tq) < kLongBwdSlices ? long_blocks(Tq) : kLongBwdSlices; }

// the workspace of the backward: D [R * H * Tq] (rounded up to a multiple of 4 floats), then the diagonal rows
size_t long_ws_dd_floats(int64_t R, int H, int Tq) { return (((size_t)R * H * Tq) + 3) / 4 * 4; }

size_t long_ws_bytes(int64_t R, int H, int Tq, int Tk) {
    return (long_ws_dd_floats(R, H, Tq) + (size_t)R * H * long_slices(Tq) * (size_t)(Tq + Tk - 1)) * sizeof(float);
}

// The checks the three entry points share, in one order; `who` names the entry point in the message.
int check_long_call(const char *who, bool train, int64_t R, int64_t Rk, int H, int d_kv, int Tq, int Tk, int past,
                    const void *anc, std::initializer_list<int64_t> strides, const float *bias, int n_delta, int bias_offset,
                    int causal, double p) {
    if (R < 0 || Rk < 0 || H < 1 || d_kv < 1 || Tq < 1 || Tk < 1) {
        set_error("%s: bad sizes (R=%lld, Rk=%lld, H=%d, d_kv=%d, Tq=%d, Tk=%d)", who, (long long)R, (long long)Rk, H, d_kv,
                  Tq, Tk);
        return RQHIP_EARG;
    }
    if (past != 0 || anc) {
        set_error("%s: past=%d / an ancestor table: the long kernel takes dense K/V with past = 0 only (the cached decode "
                  "step stays on rqhip_t5_attention)", who, past);
        return RQHIP_EUNSUPPORTED;
    }
    if (d_kv != kLongD) {
        set_error("%s: d_kv=%d, only d_kv = %d is implemented", who, d_kv, kLongD);
        return RQHIP_EUNSUPPORTED;
    }
    if (Tq > kLongMaxT || Tk > kLongMaxT) {
        set_error("%s: Tq=%d / Tk=%d exceed Tq, Tk <= %d", who, Tq, Tk, kLongMaxT);
        return RQHIP_EUNSUPPORTED;
    }
    if (train && Rk != R) {
        set_error("%s: R=%lld query rows over Rk=%lld K/V rows: the training pair takes one K/V per row (Rk = R)", who,
                  (long long)R, (long long)Rk);
        return RQHIP_EUNSUPPORTED;
    }
    if (!train && ((R > 0 && Rk == 0) || (Rk > 0 && R % Rk != 0))) {
        set_error("%s: R=%lld query rows are not a multiple of the Rk=%lld K/V groups", who, (long long)R, (long long)Rk);
        return RQHIP_EARG;
    }
    const int64_t inner = (int64_t)H * kLongD;
    for (const int64_t ld : strides) {
        if (ld < inner || ld % 4 != 0) {
            set_error("%s: row strides must be multiples of 4 and >= H * 64 = %lld (got %lld)", who, (long long)inner,
                      (long long)ld);
            return RQHIP_EARG;
        }
    }
    if (Tq > Tk && (causal || bias)) {
        set_error("%s: Tq = %d exceeds Tk = %d with causal or a bias table", who, Tq, Tk);
        return RQHIP_EARG;
    }
    const int bias_base = bias_offset - (Tq - 1);
    if (bias && (bias_base < 0 || (int64_t)bias_base + Tq + Tk - 1 > n_delta)) {
        set_error("%s: the bias table (n_delta=%d, offset=%d) does not cover deltas %d .. %d", who, n_delta, bias_offset,
                  -(Tq - 1), Tk - 1);
        return RQHIP_EARG;
    }
    if (!dropout_p_valid(p)) {
        set_error("%s: dropout probability p=%g outside 0 <= p < 1", who, p);
        return RQHIP_EARG;
    }
    const int64_t per = (int64_t)long_blocks(kLongMaxT);  // the most workgroups of a (row or group, head)
    if (Rk * (int64_t)H * per >= (1ll << 31) || R * (int64_t)H * per >= (1ll << 31)) {
        set_error("%s: R * H = %lld exceeds %lld workgroups per (row, head) within 2^31", who, (long long)(R * (int64_t)H),
                  (long long)per);
        return RQHIP_EUNSUPPORTED;
    }
    return RQHIP_OK;
}

template <auto Kernel, class... Args>
int launch_long(const char *name, size_t most, long long blocks, size_t lds, hipStream_t s, const Args &...args) {
    if (lds > 64 * 1024) {
        static LdsGrant grant;
        RQ_RETURN_IF_HIP(grant.ensure(reinterpret_cast<const void *>(Kernel), (int)most));
    }
    hipLaunchKernelGGL(Kernel, dim3((unsigned)blocks), dim3(kLongThreads), lds, s, args...);
    RQ_CHECK_LAUNCH(name);
    return RQHIP_OK;
}

LongArgs long_args(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, int64_t R, int64_t Rk, int H,
                   int Tq, int Tk, const float *bias, int bias_offset, const uint8_t *key_mask, int causal, float *out,
                   int64_t ld_out) {
    LongArgs a;
    a.q = q, a.k = k, a.v = v, a.out = out;
    a.ld_q = ld_q, a.ld_kv = ld_kv, a.ld_out = ld_out;
    a.beams = (int)(R / Rk), a.H = H, a.Tq = Tq, a.Tk = Tk, a.causal = causal != 0;
    a.nqb = long_blocks(a.beams * Tq);
    a.bias = bias, a.bias_base = bias_offset - (Tq - 1);
    a.key_mask = key_mask;
    return a;
}

// ---- the three calls, each in both arithmetics: `who` names the entry point in the messages, `bf16` picks the kernels

int long_fwd_call(const char *who, bool bf16, const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv,
                  int64_t R, int64_t Rk, int H, int d_kv, int Tq, int Tk, const float *bias_by_delta, int n_delta,
                  int bias_offset, const uint8_t *key_mask, int causal, int past, const int32_t *anc, float *out,
                  int64_t ld_out, rqhip_stream_t stream) {
    const int rc = check_long_call(who, false, R, Rk, H, d_kv, Tq, Tk, past, anc, {ld_q, ld_kv, ld_out}, bias_by_delta,
                                   n_delta, bias_offset, causal, 0.0);
    if (rc != RQHIP_OK) return rc;
    if (R == 0) return RQHIP_OK;
    if ((R / Rk) * (int64_t)Tq >= (1ll << 24)) {
        set_error("%s: %lld query rows per K/V group exceed 2^24", who, (long long)((R / Rk) * (int64_t)Tq));
        return RQHIP_EUNSUPPORTED;
    }
    if (any_null(q, k, v, out)) {
        set_error("%s: null pointer (q, k, v, out)", who);
        return RQHIP_EARG;
    }
    if (!all_aligned16(q, k, v, out)) {
        set_error("%s: q, k, v and out must be 16-byte aligned", who);
        return RQHIP_EARG;
    }
    const LongArgs a = long_args(q, ld_q, k, v, ld_kv, R, Rk, H, Tq, Tk, bias_by_delta, bias_offset, key_mask, causal, out,
                                 ld_out);
    if (Rk * (int64_t)H * a.nqb >= (1ll << 31)) {
        set_error("%s: %lld workgroups exceed 2^31", who, (long long)(Rk * (int64_t)H * a.nqb));
        return RQHIP_EUNSUPPORTED;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool has_bias = bias_by_delta != nullptr;
    if (bf16)
        return launch_long<t5_long_fwd_bf16_kernel>("t5_long_fwd_bf16_kernel",
                                                    long_fwd_lds_bytes_bf16(kLongMaxT, kLongMaxT, true), Rk * H * a.nqb,
                                                    long_fwd_lds_bytes_bf16(Tq, Tk, has_bias), s, a);
    return launch_long<t5_long_fwd_kernel>("t5_long_fwd_kernel", long_fwd_lds_bytes(kLongMaxT, kLongMaxT, true),
                                           Rk * H * a.nqb, long_fwd_lds_bytes(Tq, Tk, has_bias), s, a);
}

int long_fwd_train_call(const char *who, bool bf16, const float *q, int64_t ld_q, const float *k, const float *v,
                        int64_t ld_kv, int64_t R, int64_t Rk, int H, int d_kv, int Tq, int Tk, const float *bias_by_delta,
                        int n_delta, int bias_offset, const uint8_t *key_mask, int causal, double p, const int64_t *seed,
                        float *out, int64_t ld_out, float *lse, float *ml, rqhip_stream_t stream) {
    const int rc = check_long_call(who, true, R, Rk, H, d_kv, Tq, Tk, 0, nullptr, {ld_q, ld_kv, ld_out}, bias_by_delta,
                                   n_delta, bias_offset, causal, p);
    if (rc != RQHIP_OK) return rc;
    if (R == 0) return RQHIP_OK;
    const unsigned thresh = dropout_threshold(p);
    if (any_null(q, k, v, out, lse, ml) || (thresh && !seed)) {
        set_error("%s: null pointer (q, k, v, out, lse, ml; seed when p > 0)", who);
        return RQHIP_EARG;
    }
    if (!all_aligned16(q, k, v, out)) {
        set_error("%s: q, k, v and out must be 16-byte aligned", who);
        return RQHIP_EARG;
    }
    const LongArgs a = long_args(q, ld_q, k, v, ld_kv, R, R, H, Tq, Tk, bias_by_delta, bias_offset, key_mask, causal, out,
                                 ld_out);
    LongTrain t;
    t.lse = lse, t.ml = ml, t.seed = reinterpret_cast<const long long *>(seed), t.thresh = thresh;
    t.inv_keep = dropout_scale_f32(p);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool has_bias = bias_by_delta != nullptr;
    if (bf16)
        return launch_long<t5_long_fwd_train_bf16_kernel>("t5_long_fwd_train_bf16_kernel",
                                                          long_fwd_lds_bytes_bf16(kLongMaxT, kLongMaxT, true),
                                                          R * H * a.nqb, long_fwd_lds_bytes_bf16(Tq, Tk, has_bias), s, a, t);
    return launch_long<t5_long_fwd_train_kernel>("t5_long_fwd_train_kernel", long_fwd_lds_bytes(kLongMaxT, kLongMaxT, true),
                                                 R * H * a.nqb, long_fwd_lds_bytes(Tq, Tk, has_bias), s, a, t);
}

int long_bwd_call(const char *who, bool bf16, const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv,
                  const float *out, int64_t ld_out, const float *lse, const float *ml, const float *d_out, int64_t ld_do,
                  int64_t R, int64_t Rk, int H, int d_kv, int Tq, int Tk, const float *bias_by_delta, int n_delta,
                  int bias_offset, const uint8_t *key_mask, int causal, double p, const int64_t *seed, float *d_q,
                  float *d_k, float *d_v, float *d_bias_by_delta, void *workspace, size_t workspace_bytes,
                  rqhip_stream_t stream) {
    const int rc = check_long_call(who, true, R, Rk, H, d_kv, Tq, Tk, 0, nullptr, {ld_q, ld_kv, ld_out, ld_do},
                                   bias_by_delta, n_delta, bias_offset, causal, p);
    if (rc != RQHIP_OK) return rc;
    if (R == 0 && !bias_by_delta) return RQHIP_OK;
    const size_t need = long_ws_bytes(R, H, Tq, Tk);
    if (workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes, rqhip_t5_attention_long_bwd_workspace_bytes asks for %zu", who,
                  workspace_bytes, need);
        return RQHIP_EARG;
    }
    const unsigned thresh = dropout_threshold(p);
    if (any_null(q, k, v, out, lse, ml, d_out, d_q, d_k, d_v) || (need && !workspace) || (thresh && !seed) ||
        (bias_by_delta && !d_bias_by_delta)) {
        set_error("%s: null pointer (q, k, v, out, lse, ml, d_out, d_q, d_k, d_v, workspace; seed when p > 0; "
                  "d_bias_by_delta with a bias table)", who);
        return RQHIP_EARG;
    }
    if (!all_aligned16(q, k, v, out, d_out, d_q, d_k, d_v, workspace)) {
        set_error("%s: q, k, v, out, d_out, d_q, d_k, d_v and the workspace must be 16-byte aligned", who);
        return RQHIP_EARG;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nb = Tq + Tk - 1;
    const bool has_bias = bias_by_delta != nullptr;
    LongBwdArgs a;
    a.q = q, a.k = k, a.v = v, a.d_out = d_out, a.ml = ml;
    a.dq = d_q, a.dk = d_k, a.dv = d_v;
    a.dd = static_cast<float *>(workspace), a.dbias_part = a.dd + long_ws_dd_floats(R, H, Tq);
    a.ld_q = ld_q, a.ld_kv = ld_kv, a.ld_do = ld_do;
    a.H = H, a.Tq = Tq, a.Tk = Tk, a.causal = causal != 0;
    a.nqb = long_blocks(Tq), a.nsb = long_slices(Tq), a.nkb = long_blocks(Tk);
    a.bias = bias_by_delta, a.bias_base = bias_offset - (Tq - 1);
    a.key_mask = key_mask;
    a.seed = reinterpret_cast<const long long *>(seed), a.thresh = thresh;
    a.inv_keep = dropout_scale_f32(p);
    if (R > 0 && bf16) {
        int lrc = launch_long<t5_long_bwd_q_bf16_kernel>("t5_long_bwd_q_bf16_kernel",
                                                         long_bwd_q_lds_bytes_bf16(kLongMaxT, kLongMaxT, true),
                                                         R * H * a.nsb, long_bwd_q_lds_bytes_bf16(Tq, Tk, has_bias), s, a);
        if (lrc != RQHIP_OK) return lrc;
        lrc = launch_long<t5_long_bwd_kv_bf16_kernel>("t5_long_bwd_kv_bf16_kernel",
                                                      long_bwd_kv_lds_bytes_bf16(kLongMaxT, kLongMaxT, true), R * H * a.nkb,
                                                      long_bwd_kv_lds_bytes_bf16(Tq, Tk, has_bias), s, a);
        if (lrc != RQHIP_OK) return lrc;
    } else if (R > 0) {
        int lrc = launch_long<t5_long_bwd_q_kernel>("t5_long_bwd_q_kernel", long_bwd_q_lds_bytes(kLongMaxT, kLongMaxT, true),
                                                    R * H * a.nsb, long_bwd_q_lds_bytes(Tq, Tk, has_bias), s, a);
        if (lrc != RQHIP_OK) return lrc;
        lrc = launch_long<t5_long_bwd_kv_kernel>("t5_long_bwd_kv_kernel", long_bwd_kv_lds_bytes(kLongMaxT, kLongMaxT, true),
                                                 R * H * a.nkb, long_bwd_kv_lds_bytes(Tq, Tk, has_bias), s, a);
        if (lrc != RQHIP_OK) return lrc;
    }
    if (has_bias) {
        const long long n = (long long)n_delta * H;
        hipLaunchKernelGGL(t5_long_dbias_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.dbias_part, R,
                           H, a.nsb, nb, bias_offset - (Tq - 1), n_delta, d_bias_by_delta);
        RQ_CHECK_LAUNCH("t5_long_dbias_reduce_kernel");
    }
    return RQHIP_OK;
}

}  // namespace

}  // namespace rqhip

using namespace rqhip;

extern "C" int rqhip_t5_attention_long_supported(int d_kv, int H, int Tq, int Tk) {
    return long_supported(d_kv, H, Tq, Tk);
}

extern "C" size_t rqhip_t5_attention_long_bwd_workspace_bytes(int64_t R, int H, int Tq, int Tk) {
    if (R < 0 || H < 1 || Tq < 1 || Tk < 1) return 0;
    return long_ws_bytes(R, H, Tq, Tk);
}

#define RQ_LONG_FWD_PARAMS                                                                                              \
    const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, int64_t R, int64_t Rk, int H, int d_kv, \
        int Tq, int Tk, const float *bias_by_delta, int n_delta, int bias_offset, const uint8_t *key_mask, int causal,   \
        int past, const int32_t *anc, float *out, int64_t ld_out, rqhip_stream_t stream
#define RQ_LONG_FWD_ARGS                                                                                                   \
    q, ld_q, k, v, ld_kv, R, Rk, H, d_kv, Tq, Tk, bias_by_delta, n_delta, bias_offset, key_mask, causal, past, anc, out, \
        ld_out, stream

extern "C" int rqhip_t5_attention_long(RQ_LONG_FWD_PARAMS) {
    return long_fwd_call("t5_attention_long", false, RQ_LONG_FWD_ARGS);
}

extern "C" int rqhip_t5_attention_long_bf16(RQ_LONG_FWD_PARAMS) {
    return long_fwd_call("t5_attention_long_bf16", true, RQ_LONG_FWD_ARGS);
}

#define RQ_LONG_TRAIN_PARAMS                                                                                             \
    const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, int64_t R, int64_t Rk, int H, int d_kv, \
        int Tq, int Tk, const float *bias_by_delta, int n_delta, int bias_offset, const uint8_t *key_mask, int causal,   \
        double p, const int64_t *seed, float *out, int64_t ld_out, float *lse, float *ml, rqhip_stream_t stream
#define RQ_LONG_TRAIN_ARGS                                                                                                \
    q, ld_q, k, v, ld_kv, R, Rk, H, d_kv, Tq, Tk, bias_by_delta, n_delta, bias_offset, key_mask, causal, p, seed, out, \
        ld_out, lse, ml, stream

extern "C" int rqhip_t5_attention_long_fwd_train(RQ_LONG_TRAIN_PARAMS) {
    return long_fwd_train_call("t5_attention_long_fwd_train", false, RQ_LONG_TRAIN_ARGS);
}

extern "C" int rqhip_t5_attention_long_fwd_train_bf16(RQ_LONG_TRAIN_PARAMS) {
    return long_fwd_train_call("t5_attention_long_fwd_train_bf16", true, RQ_LONG_TRAIN_ARGS);
}

#define RQ_LONG_BWD_PARAMS                                                                                                 \
    const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, const float *out, int64_t ld_out,         \
        const float *lse, const float *ml, const float *d_out, int64_t ld_do, int64_t R, int64_t Rk, int H, int d_kv,      \
        int Tq, int Tk, const float *bias_by_delta, int n_delta, int bias_offset, const uint8_t *key_mask, int causal,     \
        double p, const int64_t *seed, float *d_q, float *d_k, float *d_v, float *d_bias_by_delta, void *workspace,        \
        size_t workspace_bytes, rqhip_stream_t stream
#define RQ_LONG_BWD_ARGS                                                                                                 \
    q, ld_q, k, v, ld_kv, out, ld_out, lse, ml, d_out, ld_do, R, Rk, H, d_kv, Tq, Tk, bias_by_delta, n_delta,          \
        bias_offset, key_mask, causal, p, seed, d_q, d_k, d_v, d_bias_by_delta, workspace, workspace_bytes, stream

extern "C" int rqhip_t5_attention_long_bwd(RQ_LONG_BWD_PARAMS) {
    return long_bwd_call("t5_attention_long_bwd", false, RQ_LONG_BWD_ARGS);
}

extern "C" int rqhip_t5_attention_long_bwd_bf16(RQ_LONG_BWD_PARAMS) {
    return long_bwd_call("t5_attention_long_bwd_bf16", true, RQ_LONG_BWD_ARGS);
}

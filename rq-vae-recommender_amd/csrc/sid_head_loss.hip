// sid_head_loss.hip -- the retrieval model's semantic-id heads and their cross-entropy losses as one call forward and
// one call backward (gfx950; modules/model.py, head_impl = "hip"; semantics in include/rqhip.h).
//
// The data is tiny (64 x 3 x 256 logits at the workload's shape) and the step is bound by launches, so there is no tile
// pipeline here: plain fp32 FMA chains on the vector ALUs, a handful of workgroups of 256 threads.
//   forward, one workgroup per (8 rows, level h): the rows' x[b, h, :] go to LDS; thread k owns code k (then k + 256,
//     ...), streams w[h][k, :] as float4 and runs eight fmaf chains in ascending j against the LDS rows (all lanes read
//     the same LDS address: a broadcast); z goes to global memory, which the backward reads again.  After a barrier
//     wave v takes rows v and v + 4: max and sum of exp over K as per-lane partials in ascending k, then an xor
//     butterfly over the 64 lanes.  A second kernel of the same call (one wave per level) adds the rows' losses in the
//     same way -- lane l holds rows l, l + 64, ... -- divides by B and adds the levels in ascending order.
//   backward, one launch with two kinds of workgroup.  (8 rows, level h): q = (exp(z - lse) - onehot) * (d_loss / B) of
//     the eight rows goes to LDS as [k][row]; thread j owns column j (then j + 256, ...) and runs eight fmaf chains in
//     ascending k over w[h][k, j] (coalesced); the workgroups of level 0 also write the zeros of positions t >= L.
//     (8 codes, level h): thread j owns column j of d_w[h][k0 .. k0 + 7, :]; the rows come in blocks of 64, whose q the
//     workgroup stages in LDS; a block is one fmaf chain in ascending b, the blocks are added in ascending order.
// No atomics and no workspace: every output element has one owner, and every order above is a function of the sizes alone.
#include <math.h>

#include "rqhip_common.h"
#include "t5_common.h"

namespace rqhip {

namespace {

constexpr int kShMaxD = 1024, kShMaxK = 1024, kShMaxL = 8;
constexpr int kShThreads = 256;
constexpr int kShRows = 8;      // rows per forward / d_x workgroup
constexpr int kShCodes = 8;     // codes per d_w workgroup
constexpr int kShDwRows = 64;   // rows per block of the d_w sum

struct ShWeights {   // the L separate [K, d] matrices, by value in the kernel's argument block
    const float *p[kShMaxL];
};
struct ShWeightGrads {
    float *p[kShMaxL];
};

bool sh_supported(int d, int K, int L) {
    return d >= 4 && d <= kShMaxD && d % 4 == 0 && K >= 1 && K <= kShMaxK && L >= 1 && L <= kShMaxL;
}

__global__ __launch_bounds__(kShThreads) void sid_head_loss_fwd_kernel(const float *x, long long ld_xb, long long ld_xt,
                                                                       ShWeights w, const long long *target,
                                                                       long long ld_t, long long B, int L, int K, int d,
                                                                       float *z, float *lse, float *row_loss) {
    __shared__ f32x4 xs[kShRows * kShMaxD / 4];
    const int h = blockIdx.y;
    const long long b0 = (long long)blockIdx.x * kShRows;
    const int nr = B - b0 < kShRows ? (int)(B - b0) : kShRows;
    const int d4 = d / 4;
    for (int i = threadIdx.x; i < kShRows * d4; i += kShThreads) {
        const int rr = i / d4, c = i - rr * d4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (rr < nr) v = *reinterpret_cast<const f32x4 *>(x + (size_t)(b0 + rr) * ld_xb + (size_t)h * ld_xt + 4 * c);
        xs[rr * d4 + c] = v;
    }
    __syncthreads();
    const float *wh = w.p[h];
    for (int k = threadIdx.x; k < K; k += kShThreads) {
        const f32x4 *wr = reinterpret_cast<const f32x4 *>(wh + (size_t)k * d);
        float acc[kShRows];
#pragma unroll
        for (int rr = 0; rr < kShRows; ++rr) acc[rr] = 0.f;
        for (int c = 0; c < d4; ++c) {
            const f32x4 wv = wr[c];
#pragma unroll
            for (int rr = 0; rr < kShRows; ++rr) {
                const f32x4 xv = xs[rr * d4 + c];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[rr] = __builtin_fmaf(xv[j], wv[j], acc[rr]);
            }
        }
#pragma unroll
        for (int rr = 0; rr < kShRows; ++rr)
            if (rr < nr) z[((size_t)(b0 + rr) * L + h) * K + k] = acc[rr];
    }
    __syncthreads();   // this workgroup's z is read back below
    const int lane = threadIdx.x & (RQ_WAVE - 1), wave = threadIdx.x / RQ_WAVE;
    for (int rr = wave; rr < nr; rr += kShThreads / RQ_WAVE) {
        const long long b = b0 + rr;
        const float *zr = z + ((size_t)b * L + h) * K;
        float m = -INFINITY;
        for (int k = lane; k < K; k += RQ_WAVE) m = fmaxf(m, zr[k]);
        m = wave_max(m);
        float s = 0.f;
        for (int k = lane; k < K; k += RQ_WAVE) s = s + expf(zr[k] - m);
        s = wave_sum(s);
        const float l = m + logf(s);
        if (lane == 0) {
            const long long t = target[(size_t)b * ld_t + h];
            lse[(size_t)b * L + h] = l;
            row_loss[(size_t)h * B + b] = (t >= 0 && t < K) ? l - zr[t] : NAN;   // never an address unchecked
        }
    }
}

// loss_d[h] = (the rows' losses: lane l adds rows l, l + 64, ... in ascending order, then the butterfly) / B; loss = the
// levels in ascending order from 0.  One workgroup of L waves.
__global__ __launch_bounds__(kShMaxL * RQ_WAVE) void sid_head_loss_mean_kernel(const float *row_loss, long long B, int L,
                                                                               float *loss_d, float *loss) {
    __shared__ float ld[kShMaxL];
    const int lane = threadIdx.x & (RQ_WAVE - 1), h = threadIdx.x / RQ_WAVE;
    float s = 0.f;
    for (long long b = lane; b < B; b += RQ_WAVE) s = s + row_loss[(size_t)h * B + b];
    s = wave_sum(s) / (float)B;
    if (lane == 0) {
        ld[h] = s;
        loss_d[h] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < L; ++i) t = t + ld[i];
        loss[0] = t;
    }
}

__device__ __forceinline__ float sh_q(const float *z, const float *lse, const long long *target, long long ld_t, int L,
                                      int K, long long b, int h, int k, float g) {
    const size_t row = (size_t)b * L + h;
    const float p = expf(z[row * K + k] - lse[row]);
    return (p - (target[(size_t)b * ld_t + h] == (long long)k ? 1.f : 0.f)) * g;
}

__global__ __launch_bounds__(kShThreads) void sid_head_loss_bwd_kernel(const float *x, long long ld_xb, long long ld_xt,
                                                                       ShWeights w, const long long *target,
                                                                       long long ld_t, const float *z, const float *lse,
                                                                       const float *d_loss, long long B, int T, int L,
                                                                       int K, int d, unsigned x_groups, float *d_x,
                                                                       ShWeightGrads d_w) {
    __shared__ f32x4 qs[kShMaxK * kShRows / 4];   // d_x: [k][8 rows]; d_w: [64 rows][8 codes]
    float *qf = reinterpret_cast<float *>(qs);
    const int h = blockIdx.y;
    const float g = d_loss[0] / (float)B;
    if (blockIdx.x < x_groups) {
        const long long b0 = (long long)blockIdx.x * kShRows;
        const int nr = B - b0 < kShRows ? (int)(B - b0) : kShRows;
        for (int i = threadIdx.x; i < kShRows * K; i += kShThreads) {
            const int rr = i / K, k = i - rr * K;
            qf[k * kShRows + rr] = rr < nr ? sh_q(z, lse, target, ld_t, L, K, b0 + rr, h, k, g) : 0.f;
        }
        __syncthreads();
        const float *wh = w.p[h];
        for (int j = threadIdx.x; j < d; j += kShThreads) {
            float acc[kShRows];
#pragma unroll
            for (int rr = 0; rr < kShRows; ++rr) acc[rr] = 0.f;
            for (int k = 0; k < K; ++k) {
                const float wv = wh[(size_t)k * d + j];
                const f32x4 q0 = qs[2 * k], q1 = qs[2 * k + 1];
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    acc[rr] = __builtin_fmaf(q0[rr], wv, acc[rr]);
                    acc[4 + rr] = __builtin_fmaf(q1[rr], wv, acc[4 + rr]);
                }
            }
#pragma unroll
            for (int rr = 0; rr < kShRows; ++rr)
                if (rr < nr) d_x[((size_t)(b0 + rr) * T + h) * d + j] = acc[rr];
            if (h == 0)   // the positions no head reads
                for (int rr = 0; rr < nr; ++rr)
                    for (int t = L; t < T; ++t) d_x[((size_t)(b0 + rr) * T + t) * d + j] = 0.f;
        }
        return;
    }
    float *dwh = d_w.p[h];
    if (!dwh) return;   // a frozen head (uniform over the workgroup)
    const int k0 = (int)(blockIdx.x - x_groups) * kShCodes;
    for (int j0 = 0; j0 < d; j0 += kShThreads) {
        const int j = j0 + threadIdx.x;
        float total[kShCodes];
#pragma unroll
        for (int i = 0; i < kShCodes; ++i) total[i] = 0.f;
        for (long long c0 = 0; c0 < B; c0 += kShDwRows) {
            const int nb = B - c0 < kShDwRows ? (int)(B - c0) : kShDwRows;
            __syncthreads();   // the previous block's q has been read
            for (int i = threadIdx.x; i < kShDwRows * kShCodes; i += kShThreads) {
                const int bb = i / kShCodes, k = k0 + i % kShCodes;
                qf[i] = (bb < nb && k < K) ? sh_q(z, lse, target, ld_t, L, K, c0 + bb, h, k, g) : 0.f;
            }
            __syncthreads();
            if (j < d) {
                float acc[kShCodes];
#pragma unroll
                for (int i = 0; i < kShCodes; ++i) acc[i] = 0.f;
                for (int bb = 0; bb < nb; ++bb) {
                    const float xv = x[(size_t)(c0 + bb) * ld_xb + (size_t)h * ld_xt + j];
                    const f32x4 q0 = qs[2 * bb], q1 = qs[2 * bb + 1];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        acc[i] = __builtin_fmaf(q0[i], xv, acc[i]);
                        acc[4 + i] = __builtin_fmaf(q1[i], xv, acc[4 + i]);
                    }
                }
#pragma unroll
                for (int i = 0; i < kShCodes; ++i) total[i] = total[i] + acc[i];
            }
        }
        if (j < d) {
#pragma unroll
            for (int i = 0; i < kShCodes; ++i)
                if (k0 + i < K) dwh[(size_t)(k0 + i) * d + j] = total[i];
        }
    }
}

// The checks both entry points share; `who` names the entry point in the message.
int sh_check(const char *who, int64_t B, int T, int L, int K, int d, int64_t ld_xb, int64_t ld_xt, int64_t ld_t) {
    if (B < 1 || T < 0 || L < 0 || K < 0 || d < 0) {
        set_error("%s: bad sizes (B=%lld, T=%d, L=%d, K=%d, d=%d)", who, (long long)B, T, L, K, d);
        return RQHIP_EARG;
    }
    if (!sh_supported(d, K, L)) {
        set_error("%s: d=%d, K=%d, L=%d: only d a multiple of 4 in 4 .. %d, K in 1 .. %d and L in 1 .. %d are implemented",
                  who, d, K, L, kShMaxD, kShMaxK, kShMaxL);
        return RQHIP_EUNSUPPORTED;
    }
    if (T < L) {
        set_error("%s: T=%d positions per row, fewer than the L=%d levels", who, T, L);
        return RQHIP_EARG;
    }
    if (ld_t < L) {
        set_error("%s: target row stride %lld below L=%d", who, (long long)ld_t, L);
        return RQHIP_EARG;
    }
    if (ld_xb < 0 || ld_xt < 0 || ld_xb % 4 || ld_xt % 4) {
        set_error("%s: x strides (%lld per row, %lld per position) must be non-negative multiples of 4 elements: x rows "
                  "are read as 16-byte aligned float4", who, (long long)ld_xb, (long long)ld_xt);
        return RQHIP_EARG;
    }
    if ((B + kShRows - 1) / kShRows >= (1ll << 31)) {
        set_error("%s: B=%lld exceeds %d rows per workgroup of a 2^31 grid", who, (long long)B, kShRows);
        return RQHIP_EUNSUPPORTED;
    }
    return RQHIP_OK;
}

}  // namespace

}  // namespace rqhip

using namespace rqhip;

extern "C" int rqhip_sid_head_loss_supported(int d, int K, int L) { return sh_supported(d, K, L); }

extern "C" int rqhip_sid_head_loss_fwd(const float *x, int64_t ld_xb, int64_t ld_xt, const float *const *w,
                                       const int64_t *target, int64_t ld_t, int64_t B, int T, int L, int K, int d,
                                       float *z, float *lse, float *row_loss, float *loss_d, float *loss,
                                       rqhip_stream_t stream) {
    const char *who = "sid_head_loss_fwd";
    const int rc = sh_check(who, B, T, L, K, d, ld_xb, ld_xt, ld_t);
    if (rc != RQHIP_OK) return rc;
    bool null = any_null(x, w, target, z, lse, row_loss, loss_d, loss);
    ShWeights ws = {};
    for (int h = 0; h < L && !null; ++h) null = !(ws.p[h] = w[h]);
    if (null) {
        set_error("%s: null pointer (x, w and its L entries, target, z, lse, row_loss, loss_d, loss)", who);
        return RQHIP_EARG;
    }
    bool aligned = aligned16(x);
    for (int h = 0; h < L; ++h) aligned = aligned && aligned16(ws.p[h]);
    if (!aligned) {
        set_error("%s: x and every w[h] must be 16-byte aligned", who);
        return RQHIP_EARG;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sid_head_loss_fwd_kernel, dim3((unsigned)((B + kShRows - 1) / kShRows), (unsigned)L),
                       dim3(kShThreads), 0, s, x, (long long)ld_xb, (long long)ld_xt, ws,
                       reinterpret_cast<const long long *>(target), (long long)ld_t, (long long)B, L, K, d, z, lse,
                       row_loss);
    RQ_CHECK_LAUNCH("sid_head_loss_fwd_kernel");
    hipLaunchKernelGGL(sid_head_loss_mean_kernel, dim3(1), dim3((unsigned)(L * RQ_WAVE)), 0, s, row_loss, (long long)B, L,
                       loss_d, loss);
    RQ_CHECK_LAUNCH("sid_head_loss_mean_kernel");
    return RQHIP_OK;
}

extern "C" int rqhip_sid_head_loss_bwd(const float *x, int64_t ld_xb, int64_t ld_xt, const float *const *w,
                                       const int64_t *target, int64_t ld_t, const float *z, const float *lse,
                                       const float *d_loss, int64_t B, int T, int L, int K, int d, float *d_x,
                                       float *const *d_w, rqhip_stream_t stream) {
    const char *who = "sid_head_loss_bwd";
    const int rc = sh_check(who, B, T, L, K, d, ld_xb, ld_xt, ld_t);
    if (rc != RQHIP_OK) return rc;
    bool null = any_null(x, w, target, z, lse, d_loss);
    ShWeights ws = {};
    for (int h = 0; h < L && !null; ++h) null = !(ws.p[h] = w[h]);
    if (null) {
        set_error("%s: null pointer (x, w and its L entries, target, z, lse, d_loss)", who);
        return RQHIP_EARG;
    }
    if (!aligned16(x)) {
        set_error("%s: x must be 16-byte aligned", who);
        return RQHIP_EARG;
    }
    ShWeightGrads gs = {};
    bool any_w = false;
    for (int h = 0; h < L && d_w; ++h) any_w = (gs.p[h] = d_w[h]) || any_w;
    if (!d_x && !any_w) return RQHIP_OK;   // nothing is wanted
    const unsigned x_groups = d_x ? (unsigned)((B + kShRows - 1) / kShRows) : 0u;
    const unsigned w_groups = any_w ? (unsigned)((K + kShCodes - 1) / kShCodes) : 0u;
    hipLaunchKernelGGL(sid_head_loss_bwd_kernel, dim3(x_groups + w_groups, (unsigned)L), dim3(kShThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), x, (long long)ld_xb, (long long)ld_xt, ws,
                       reinterpret_cast<const long long *>(target), (long long)ld_t, z, lse, d_loss, (long long)B, T, L, K,
                       d, x_groups, d_x, gs);
    RQ_CHECK_LAUNCH("sid_head_loss_bwd_kernel");
    return RQHIP_OK;
}

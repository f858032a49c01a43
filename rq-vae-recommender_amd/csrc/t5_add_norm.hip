// t5_add_norm.hip -- the glue between two T5 sub-layers as one launch (gfx950): the dropout of a sub-layer's output, the
// residual add, the next RMS norm and, behind the final norm, its dropout (modules/t5.py; semantics in include/rqhip.h).
//
// One wave64 owns one row [d], d % 4 == 0, d <= 1024: lane l holds the float4s l, l + 64, l + 128, l + 192 of the row
// in registers.  A row sum is the lane's elements in ascending order, then an xor butterfly over the 64 lanes (32, 16,
// 8, 4, 2, 1): its order is a function of d alone, and every lane ends with the same bits.  The forward has no LDS and
// no barrier.  In the backward a workgroup owns a contiguous range of rows, its four waves take every fourth row of it
// and keep the weight gradient's per-column sums in registers; the waves' sums are added in wave order through LDS into
// one partial block [d] per workgroup, and a second kernel adds the blocks in ascending order: no atomics, and a row
// partition that depends on (N, d) only, so d_w has the same bits on every run and every device.
#include <math.h>

#include "rqhip_common.h"
#include "t5_common.h"

namespace rqhip {

namespace {

constexpr int kAnMaxD = 1024;
constexpr int kAnWaves = 4;       // waves (forward: rows) per workgroup
constexpr int kAnBwdRows = 64;    // rows per backward workgroup up to kAnMaxBlocks blocks, then doubled until they fit
constexpr int kAnMaxBlocks = 256;

bool an_supported(int d) { return d >= 4 && d <= kAnMaxD && d % 4 == 0; }

long long an_bwd_rows(long long N) {
    long long rows = kAnBwdRows;
    while ((N + rows - 1) / rows > kAnMaxBlocks) rows *= 2;
    return rows;
}

long long an_bwd_blocks(long long N) {
    const long long rows = an_bwd_rows(N);
    return N > 0 ? (N + rows - 1) / rows : 1;
}

struct AnDrop {
    const long long *seed;    // one int64 on the device (read only when a threshold is non-zero)
    unsigned th_in, th_out;   // round(p * 2^32); 0 = no dropout
    float s_in, s_out;        // 1 / (1 - p)
};

__global__ __launch_bounds__(kAnWaves * RQ_WAVE) void t5_add_norm_fwd_kernel(const float *x, const float *y, const float *w,
                                                                             long long N, int d, float eps, AnDrop dr,
                                                                             float *x_new, float *n, float *rstd) {
    const int lane = threadIdx.x & (RQ_WAVE - 1), wave = threadIdx.x / RQ_WAVE;
    const long long row = (long long)blockIdx.x * kAnWaves + wave;
    if (row >= N) return;  // a whole wave: the shuffles below stay among live lanes
    const unsigned long long seed = (dr.th_in | dr.th_out) ? (unsigned long long)*dr.seed : 0ull;
    const unsigned long long e0 = (unsigned long long)row * (unsigned long long)d;
    const unsigned long long plane = (unsigned long long)N * (unsigned long long)d;
    const size_t base = (size_t)row * (size_t)d;

    f32x4 v[4];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = 4 * (lane + RQ_WAVE * k);
        v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < d) {
            f32x4 t = *reinterpret_cast<const f32x4 *>(y + base + c);
            if (dr.th_in) {
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = dropout_keep(seed, e0 + c + j, dr.th_in) ? t[j] * dr.s_in : 0.f;
            }
            if (x) {
                const f32x4 xx = *reinterpret_cast<const f32x4 *>(x + base + c);
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = xx[j] + t[j];
            }
            *reinterpret_cast<f32x4 *>(x_new + base + c) = t;
            v[k] = t;
#pragma unroll
            for (int j = 0; j < 4; ++j) ss = ss + t[j] * t[j];
        }
    }
    ss = wave_sum(ss);
    const float r = 1.0f / sqrtf(ss / (float)d + eps);
    if (lane == 0) rstd[row] = r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = 4 * (lane + RQ_WAVE * k);
        if (c < d) {
            const f32x4 ww = *reinterpret_cast<const f32x4 *>(w + c);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = ww[j] * (v[k][j] * r);
                if (dr.th_out) o[j] = dropout_keep(seed, plane + e0 + c + j, dr.th_out) ? o[j] * dr.s_out : 0.f;
            }
            *reinterpret_cast<f32x4 *>(n + base + c) = o;
        }
    }
}

__global__ __launch_bounds__(kAnWaves * RQ_WAVE) void t5_add_norm_bwd_kernel(const float *x_new, const float *rstd,
                                                                             const float *w, const float *d_n,
                                                                             const float *d_xnew, long long N, int d,
                                                                             long long rows_per_wg, AnDrop dr, float *d_x,
                                                                             float *d_y, float *part) {
    __shared__ float sums[kAnWaves * kAnMaxD];
    const int lane = threadIdx.x & (RQ_WAVE - 1), wave = threadIdx.x / RQ_WAVE;
    const unsigned long long seed = (dr.th_in | dr.th_out) ? (unsigned long long)*dr.seed : 0ull;
    const unsigned long long plane = (unsigned long long)N * (unsigned long long)d;
    const long long row0 = (long long)blockIdx.x * rows_per_wg;
    const long long row1 = row0 + rows_per_wg < N ? row0 + rows_per_wg : N;

    f32x4 ww[4], acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = 4 * (lane + RQ_WAVE * k);
        acc[k] = ww[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < d) ww[k] = *reinterpret_cast<const f32x4 *>(w + c);
    }
    for (long long row = row0 + wave; row < row1; row += kAnWaves) {
        const unsigned long long e0 = (unsigned long long)row * (unsigned long long)d;
        const size_t base = (size_t)row * (size_t)d;
        const float r = rstd[row];
        f32x4 gw[4], xh[4];
        float cs = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = 4 * (lane + RQ_WAVE * k);
            gw[k] = xh[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c < d) {
                const f32x4 xn = *reinterpret_cast<const f32x4 *>(x_new + base + c);
                f32x4 g = {0.f, 0.f, 0.f, 0.f};
                if (d_n) g = *reinterpret_cast<const f32x4 *>(d_n + base + c);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (dr.th_out) g[j] = g[j] * (dropout_keep(seed, plane + e0 + c + j, dr.th_out) ? dr.s_out : 0.f);
                    xh[k][j] = xn[j] * r;
                    gw[k][j] = g[j] * ww[k][j];
                    acc[k][j] = acc[k][j] + g[j] * xh[k][j];
                    cs = cs + gw[k][j] * xh[k][j];
                }
            }
        }
        const float cm = wave_sum(cs) / (float)d;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = 4 * (lane + RQ_WAVE * k);
            if (c < d) {
                f32x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = r * (gw[k][j] - xh[k][j] * cm);
                if (d_xnew) {
                    const f32x4 up = *reinterpret_cast<const f32x4 *>(d_xnew + base + c);
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = up[j] + o[j];
                }
                if (d_x) *reinterpret_cast<f32x4 *>(d_x + base + c) = o;
                if (d_y) {
                    if (dr.th_in) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) o[j] = dropout_keep(seed, e0 + c + j, dr.th_in) ? o[j] * dr.s_in : 0.f;
                    }
                    *reinterpret_cast<f32x4 *>(d_y + base + c) = o;
                }
            }
        }
    }
    // the waves' column sums in wave order -> this workgroup's partial block
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = 4 * (lane + RQ_WAVE * k);
        if (c < d) *reinterpret_cast<f32x4 *>(sums + wave * d + c) = acc[k];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += kAnWaves * RQ_WAVE) {
        float s = sums[c];
#pragma unroll
        for (int wv = 1; wv < kAnWaves; ++wv) s = s + sums[wv * d + c];
        part[(size_t)blockIdx.x * (size_t)d + c] = s;
    }
}

// d_w[c] = the partial blocks in ascending order (zero without rows)
__global__ __launch_bounds__(256) void t5_add_norm_dw_kernel(const float *part, long long blocks, int d, float *d_w) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= d) return;
    float s = 0.f;
    if (blocks > 0) s = part[c];
    for (long long b = 1; b < blocks; ++b) s = s + part[(size_t)b * (size_t)d + c];
    d_w[c] = s;
}

// The checks both entry points share; `who` names the entry point in the message.
int an_check(const char *who, int64_t N, int d, double p_in, double p_out) {
    if (N < 0 || d < 1) {
        set_error("%s: bad sizes (N=%lld, d=%d)", who, (long long)N, d);
        return RQHIP_EARG;
    }
    if (!dropout_p_valid(p_in) || !dropout_p_valid(p_out)) {
        set_error("%s: dropout probabilities p_in=%g, p_out=%g outside 0 <= p < 1", who, p_in, p_out);
        return RQHIP_EARG;
    }
    if (!an_supported(d)) {
        set_error("%s: d=%d, only multiples of 4 in 4 .. %d are implemented", who, d, kAnMaxD);
        return RQHIP_EUNSUPPORTED;
    }
    if ((N + kAnWaves - 1) / kAnWaves >= (1ll << 31)) {
        set_error("%s: N=%lld exceeds %d rows per workgroup of a 2^31 grid", who, (long long)N, kAnWaves);
        return RQHIP_EUNSUPPORTED;
    }
    return RQHIP_OK;
}

AnDrop an_drop(double p_in, double p_out, const int64_t *seed) {
    AnDrop dr;
    dr.seed = reinterpret_cast<const long long *>(seed);
    dr.th_in = dropout_threshold(p_in), dr.th_out = dropout_threshold(p_out);
    dr.s_in = dropout_scale_f64(p_in), dr.s_out = dropout_scale_f64(p_out);
    return dr;
}

}  // namespace

}  // namespace rqhip

using namespace rqhip;

extern "C" int rqhip_t5_add_norm_supported(int d) { return an_supported(d); }

extern "C" size_t rqhip_t5_add_norm_bwd_workspace_bytes(int64_t N, int d) {
    if (N < 0 || !an_supported(d)) return 0;
    return (size_t)an_bwd_blocks(N) * (size_t)d * sizeof(float);
}

extern "C" int rqhip_t5_add_norm_fwd(const float *x, const float *y, const float *w, int64_t N, int d, float eps,
                                     double p_in, double p_out, const int64_t *seed, float *x_new, float *n, float *rstd,
                                     rqhip_stream_t stream) {
    const int rc = an_check("t5_add_norm_fwd", N, d, p_in, p_out);
    if (rc != RQHIP_OK) return rc;
    if (N == 0) return RQHIP_OK;
    const AnDrop dr = an_drop(p_in, p_out, seed);
    if (any_null(y, w, x_new, n, rstd) || ((dr.th_in | dr.th_out) && !seed)) {
        set_error("t5_add_norm_fwd: null pointer (y, w, x_new, n, rstd; seed when p_in > 0 or p_out > 0)");
        return RQHIP_EARG;
    }
    if (!all_aligned16(x, y, w, x_new, n)) {
        set_error("t5_add_norm_fwd: x, y, w, x_new and n must be 16-byte aligned");
        return RQHIP_EARG;
    }
    hipLaunchKernelGGL(t5_add_norm_fwd_kernel, dim3((unsigned)((N + kAnWaves - 1) / kAnWaves)), dim3(kAnWaves * RQ_WAVE), 0,
                       reinterpret_cast<hipStream_t>(stream), x, y, w, (long long)N, d, eps, dr, x_new, n, rstd);
    RQ_CHECK_LAUNCH("t5_add_norm_fwd_kernel");
    return RQHIP_OK;
}

extern "C" int rqhip_t5_add_norm_bwd(const float *x_new, const float *rstd, const float *w, const float *d_n,
                                     const float *d_xnew, int64_t N, int d, double p_in, double p_out, const int64_t *seed,
                                     float *d_x, float *d_y, float *d_w, void *workspace, size_t workspace_bytes,
                                     rqhip_stream_t stream) {
    const int rc = an_check("t5_add_norm_bwd", N, d, p_in, p_out);
    if (rc != RQHIP_OK) return rc;
    if (N == 0 && !d_w) return RQHIP_OK;
    const AnDrop dr = an_drop(p_in, p_out, seed);
    if (!d_w || (N > 0 && (any_null(x_new, rstd, w) || ((dr.th_in | dr.th_out) && !seed)))) {
        set_error("t5_add_norm_bwd: null pointer (x_new, rstd, w, d_w; seed when p_in > 0 or p_out > 0)");
        return RQHIP_EARG;
    }
    if (!all_aligned16(x_new, w, d_n, d_xnew, d_x, d_y)) {
        set_error("t5_add_norm_bwd: x_new, w, d_n, d_xnew, d_x and d_y must be 16-byte aligned");
        return RQHIP_EARG;
    }
    const long long blocks = N > 0 ? an_bwd_blocks(N) : 0;
    if (N > 0 && (!workspace || workspace_bytes < rqhip_t5_add_norm_bwd_workspace_bytes(N, d))) {
        set_error("t5_add_norm_bwd: workspace of %zu bytes, rqhip_t5_add_norm_bwd_workspace_bytes(N, d) = %zu",
                  workspace_bytes, rqhip_t5_add_norm_bwd_workspace_bytes(N, d));
        return RQHIP_EARG;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float *part = reinterpret_cast<float *>(workspace);
    if (N > 0) {
        hipLaunchKernelGGL(t5_add_norm_bwd_kernel, dim3((unsigned)blocks), dim3(kAnWaves * RQ_WAVE), 0, s, x_new, rstd, w, d_n,
                           d_xnew, (long long)N, d, an_bwd_rows(N), dr, d_x, d_y, part);
        RQ_CHECK_LAUNCH("t5_add_norm_bwd_kernel");
    }
    hipLaunchKernelGGL(t5_add_norm_dw_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, part, blocks, d, d_w);
    RQ_CHECK_LAUNCH("t5_add_norm_dw_kernel");
    return RQHIP_OK;
}

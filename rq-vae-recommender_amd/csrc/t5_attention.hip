// t5_attention.hip -- one T5 attention call of the retrieval model's inference path as one launch (gfx950).
//
// modules/t5.py:_attend is a matmul, up to two adds, an fp32 softmax and a second matmul around head transposes, and
// writes a [R, H, Tq, Tk] score tensor.  Here one workgroup owns one (K/V group, head): it stages that head's K and V
// rows [Tk, 64] in LDS ONCE (row stride 68 floats: both operand reads below hit 64 distinct banks) and its waves take
// the group's beams * Tq query rows sixteen at a time.  Everything is fp32 on v_mfma_f32_16x16x4_f32; T5 semantics:
// no 1/sqrt(d) scaling, d_kv = 64, masked scores get finfo(float32).min ADDED (a row with every key masked is the
// uniform average of V, as with the operators).
//
// Both products are computed transposed, so that the scores never leave their registers:
//   S^T = K Q^T   A: lane (key jj, slot g) = K[16 mt + jj][4 e + g] (LDS), B: lane (slot g, query i) = Q[i][4 e + g]
//                 (global, 16 registers per tile), e = 0..15.  Lane (g, i) ends with S[i][16 mt + 4 g + r], r = 0..3.
//   softmax over the keys of query i: the lane's own registers in (mt, r) order, then lanes g (xor 16, xor 32).
//   O^T = V^T P^T instruction (mt, r) takes key 16 mt + 4 g + r as its reduction slot g: B is the lane's OWN register
//                 p[mt][r], A: lane (d dd, slot g) = V[16 mt + 4 g + r][16 dt + dd] (LDS).  Lane (g, i) ends with
//                 O[i][16 dt + 4 g + 0..3]: one 16-byte store per dt, after one IEEE divide by the row's sum.
// q is read as the q Linear wrote it ([R, Tq, H * 64]) and the output is written as o reads it: no transposes.
//
// K/V sources: dense [Rk, Tk, H * 64] (rows b * beams .. b * beams + beams - 1 of q read group b), or, for the cached
// decode step (Tq = 1, Rk = R), per-position slabs [t][slab_rows, H * 64] through the ancestor table anc [R, past]:
// key t < past of row r is row anc[r, t] of slab t, key `past` is row r of slab `past`.  Nothing is copied.
//
// Fixed reduction orders, no atomics, no host sync: the same bits on every run; graph-capturable once the LDS
// attribute has been raised by a first eager call, as everywhere in this library.
#include <float.h>

#include "rqhip_common.h"

namespace rqhip {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kAttD = 64;       // d_kv
constexpr int kAttLd = 68;      // LDS row stride of K and V (floats)
constexpr int kAttMaxT = 256;   // Tq, Tk

struct AttArgs {
    const float *q, *k, *v;
    float *out;
    long long ld_q, ld_kv, ld_out;
    int beams, H, Tq, Tk, past, causal;
    const float *bias;  // [n_delta, H] or null
    int bias_base;      // table row of delta = -(Tq - 1) - past
    const unsigned char *key_mask;  // [Rk, Tk] or null
    const int *anc;     // [R, ld_anc] or null (dense K/V)
    long long ld_anc, slab_rows;
};

template <int MT>
__global__ __launch_bounds__(256) void t5_attention_kernel(AttArgs a) {
    extern __shared__ float att_lds[];
    const int ntiles = (a.Tk + 15) >> 4, Tkp = ntiles << 4;
    float *Ks = att_lds;
    float *Vs = Ks + (size_t)Tkp * kAttLd;
    float *madd = Vs + (size_t)Tkp * kAttLd;  // 0: kept, -FLT_MAX: masked, -inf: padding beyond Tk
    float *bias_s = madd + Tkp;               // [Tq + Tk - 1] of this head, by j - i + Tq - 1

    const long long b = blockIdx.x / a.H;
    const int h = blockIdx.x - (int)b * a.H;
    const int tid = threadIdx.x, nthr = blockDim.x;

    // ---- stage K, V (zeros beyond Tk: 0 * p must stay 0), the key mask and the head's bias column
    for (int idx = tid; idx < Tkp * 16; idx += nthr) {
        const int j = idx >> 4, c = idx & 15;
        float4 kk = make_float4(0.f, 0.f, 0.f, 0.f), vv = kk;
        if (j < a.Tk) {
            long long tok;
            if (a.anc) {
                long long row = b;
                if (j < a.past) {
                    row = a.anc[b * a.ld_anc + j];
                    row = row < 0 ? 0 : (row >= a.slab_rows ? a.slab_rows - 1 : row);
                }
                tok = (long long)j * a.slab_rows + row;
            } else {
                tok = b * a.Tk + j;
            }
            const size_t off = (size_t)tok * (size_t)a.ld_kv + (size_t)h * kAttD + 4 * c;
            kk = *reinterpret_cast<const float4 *>(a.k + off);
            vv = *reinterpret_cast<const float4 *>(a.v + off);
        }
        *reinterpret_cast<float4 *>(Ks + j * kAttLd + 4 * c) = kk;
        *reinterpret_cast<float4 *>(Vs + j * kAttLd + 4 * c) = vv;
    }
    for (int j = tid; j < Tkp; j += nthr)
        madd[j] = j >= a.Tk ? -INFINITY : ((a.key_mask && !a.key_mask[b * a.Tk + j]) ? -FLT_MAX : 0.f);
    if (a.bias)
        for (int x = tid; x < a.Tq + a.Tk - 1; x += nthr) bias_s[x] = a.bias[(size_t)(a.bias_base + x) * a.H + h];
    __syncthreads();

    const int nw = nthr / RQ_WAVE, wave = tid / RQ_WAVE, lane = tid & (RQ_WAVE - 1);
    const int i = lane & 15, g = lane >> 4;
    const int M = a.beams * a.Tq;
    for (int qt = wave; qt * 16 < M; qt += nw) {
        const int m = qt * 16 + i;
        const int mc = m < M ? m : M - 1;  // lanes past the last query recompute it and store nothing
        const int beam = mc / a.Tq, ti = mc - beam * a.Tq;
        const size_t qrow = (size_t)(b * a.beams + beam) * (size_t)a.Tq + (size_t)ti;
        const float *qp = a.q + qrow * (size_t)a.ld_q + (size_t)h * kAttD + g;
        float qreg[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) qreg[e] = qp[4 * e];

        // ---- scores, bias, masks
        f32x4 s[MT];
        float mx = -INFINITY;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            s[mt] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (mt < ntiles) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                const float *kp = Ks + (16 * mt + i) * kAttLd + g;
#pragma unroll
                for (int e = 0; e < 16; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kp[4 * e], qreg[e], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 16 * mt + 4 * g + r;
                    const float ma = madd[j];
                    float sc = acc[r];
                    if (ma == -INFINITY) {
                        sc = -INFINITY;
                    } else {
                        if (a.bias) sc = sc + bias_s[j - ti + a.Tq - 1];
                        if (ma != 0.f || (a.causal && j > ti + a.past)) sc = sc + -FLT_MAX;
                    }
                    s[mt][r] = sc;
                    mx = fmaxf(mx, sc);
                }
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, RQ_WAVE));
        mx = fmaxf(mx, __shfl_xor(mx, 32, RQ_WAVE));

        // ---- exp and the row sum (the lane's keys in order, then the four lanes of the query)
        float sum = 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (mt < ntiles) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = expf(s[mt][r] - mx);
                    s[mt][r] = p;
                    sum = sum + p;
                }
            }
        }
        sum = sum + __shfl_xor(sum, 16, RQ_WAVE);
        sum = sum + __shfl_xor(sum, 32, RQ_WAVE);

        // ---- O^T = V^T P^T
        f32x4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (mt < ntiles) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float *vp = Vs + (16 * mt + 4 * g + r) * kAttLd + i;
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt)
                        o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[16 * dt], s[mt][r], o[dt], 0, 0, 0);
                }
            }
        }
        if (m < M) {
            float *op = a.out + qrow * (size_t)a.ld_out + (size_t)h * kAttD + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<float4 *>(op + 16 * dt) =
                    make_float4(o[dt][0] / sum, o[dt][1] / sum, o[dt][2] / sum, o[dt][3] / sum);
        }
    }
}

size_t att_lds_bytes(int Tq, int Tk, bool bias) {
    const size_t Tkp = (size_t)((Tk + 15) / 16) * 16;
    return (2 * Tkp * kAttLd + Tkp + (bias ? (size_t)(Tq + Tk - 1) : 0)) * sizeof(float);
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int MT>
int launch_att(const AttArgs &a, long long groups, int threads, size_t lds, hipStream_t s) {
    if (lds > 64 * 1024) {
        // the grant is made once per device and never raised again: ask for the most this instantiation can need
        static LdsGrant grant;
        RQ_RETURN_IF_HIP(grant.ensure(reinterpret_cast<const void *>(t5_attention_kernel<MT>),
                                      (int)att_lds_bytes(kAttMaxT, MT * 16 < kAttMaxT ? MT * 16 : kAttMaxT, true)));
    }
    hipLaunchKernelGGL(t5_attention_kernel<MT>, dim3((unsigned)(groups * a.H)), dim3(threads), lds, s, a);
    RQ_CHECK_LAUNCH("t5_attention_kernel");
    return RQHIP_OK;
}

}  // namespace

}  // namespace rqhip

using namespace rqhip;

extern "C" int rqhip_t5_attention_supported(int d_kv, int H, int Tq, int Tk) {
    return d_kv == kAttD && H >= 1 && Tq >= 1 && Tq <= kAttMaxT && Tk >= 1 && Tk <= kAttMaxT;
}

extern "C" int rqhip_t5_attention(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, int64_t R,
                                  int64_t Rk, int H, int d_kv, int Tq, int Tk, const float *bias_by_delta, int n_delta,
                                  int bias_offset, const uint8_t *key_mask, int causal, int past, const int32_t *anc,
                                  int64_t ld_anc, int64_t slab_rows, float *out, int64_t ld_out,
                                  rqhip_stream_t stream) {
    if (R < 0 || Rk < 0 || H < 1 || d_kv < 1 || Tq < 1 || Tk < 1 || past < 0) {
        set_error("t5_attention: bad sizes (R=%lld, Rk=%lld, H=%d, d_kv=%d, Tq=%d, Tk=%d, past=%d)", (long long)R,
                  (long long)Rk, H, d_kv, Tq, Tk, past);
        return RQHIP_EARG;
    }
    if (d_kv != kAttD) {
        set_error("t5_attention: d_kv=%d, only d_kv = %d is implemented", d_kv, kAttD);
        return RQHIP_EUNSUPPORTED;
    }
    if (Tq > kAttMaxT || Tk > kAttMaxT) {
        set_error("t5_attention: Tq=%d / Tk=%d exceed Tq, Tk <= %d", Tq, Tk, kAttMaxT);
        return RQHIP_EUNSUPPORTED;
    }
    if ((R > 0 && Rk == 0) || (Rk > 0 && R % Rk != 0)) {
        set_error("t5_attention: R=%lld query rows are not a multiple of the Rk=%lld K/V groups", (long long)R,
                  (long long)Rk);
        return RQHIP_EARG;
    }
    const int64_t inner = (int64_t)H * kAttD;
    if (ld_q < inner || ld_kv < inner || ld_out < inner || (ld_q | ld_kv | ld_out) % 4 != 0) {
        set_error("t5_attention: row strides (q %lld, k/v %lld, out %lld) must be multiples of 4 and >= H * 64 = %lld",
                  (long long)ld_q, (long long)ld_kv, (long long)ld_out, (long long)inner);
        return RQHIP_EARG;
    }
    if (anc) {
        if (Tq != 1 || Rk != R || Tk != past + 1 || ld_anc < past || slab_rows < R) {
            set_error("t5_attention: the ancestor table takes Tq = 1, Rk = R, Tk = past + 1, ld_anc >= past and "
                      "slab_rows >= R (Tq=%d, R=%lld, Rk=%lld, Tk=%d, past=%d, ld_anc=%lld, slab_rows=%lld)",
                      Tq, (long long)R, (long long)Rk, Tk, past, (long long)ld_anc, (long long)slab_rows);
            return RQHIP_EARG;
        }
    } else if (past + Tq > Tk && (causal || bias_by_delta)) {
        set_error("t5_attention: past + Tq = %d exceeds Tk = %d", past + Tq, Tk);
        return RQHIP_EARG;
    }
    const int bias_base = bias_offset - (Tq - 1) - past;  // table row of the smallest delta j - i - past
    if (bias_by_delta && (bias_base < 0 || (int64_t)bias_base + Tq + Tk - 1 > n_delta)) {
        set_error("t5_attention: the bias table (n_delta=%d, offset=%d) does not cover deltas %d .. %d", n_delta,
                  bias_offset, -(Tq - 1) - past, Tk - 1 - past);
        return RQHIP_EARG;
    }
    if (Rk * (int64_t)H >= (1ll << 31)) {
        set_error("t5_attention: Rk * H = %lld exceeds one workgroup per (group, head) (< 2^31)",
                  (long long)(Rk * (int64_t)H));
        return RQHIP_EUNSUPPORTED;
    }
    if (R == 0) return RQHIP_OK;
    if (!q || !k || !v || !out) {
        set_error("t5_attention: null pointer (q, k, v, out)");
        return RQHIP_EARG;
    }
    if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out)) {
        set_error("t5_attention: q, k, v and out must be 16-byte aligned");
        return RQHIP_EARG;
    }

    AttArgs a;
    a.q = q, a.k = k, a.v = v, a.out = out;
    a.ld_q = ld_q, a.ld_kv = ld_kv, a.ld_out = ld_out;
    a.beams = (int)(R / Rk), a.H = H, a.Tq = Tq, a.Tk = Tk, a.past = past, a.causal = causal != 0;
    a.bias = bias_by_delta, a.bias_base = bias_base;
    a.key_mask = key_mask;
    a.anc = past > 0 ? anc : nullptr;  // at past = 0 the only key is the row's own: the dense form of slab 0
    a.ld_anc = ld_anc, a.slab_rows = slab_rows;
    if ((int64_t)a.beams * Tq >= (1ll << 24)) {
        set_error("t5_attention: %lld query rows per K/V group", (long long)a.beams * Tq);
        return RQHIP_EUNSUPPORTED;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = att_lds_bytes(Tq, Tk, bias_by_delta != nullptr);
    const int ntiles = (Tk + 15) / 16;
    if (ntiles == 1) return launch_att<1>(a, Rk, RQ_WAVE, lds, s);
    if (ntiles <= 6) return launch_att<6>(a, Rk, 4 * RQ_WAVE, lds, s);
    return launch_att<16>(a, Rk, 4 * RQ_WAVE, lds, s);
}

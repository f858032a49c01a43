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
// Or packed [n_k, H * 64] behind a cumulative table (the PACKED instantiations): a group's own length gives its loops,
// with one K/V per query group, or, for a decode step's cross-attention over packed encoder rows, the beams as above.
//
// Fixed reduction orders, no atomics, no host sync: the same bits on every run; graph-capturable once the LDS
// attribute has been raised by a first eager call, as everywhere in this library.
#include <float.h>
#include <math.h>

#include <initializer_list>
#include <type_traits>

#include "rqhip_common.h"
#include "t5_common.h"

namespace rqhip {

namespace {

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
    const int *cu_q, *cu_k;  // the packed kernels' cumulative row tables [groups + 1], each may be null (that side dense)
    long long n_q, n_k;      // rows of the packed q / out and k / v tensors
};

// What the training forward adds to a call: the row log-sum-exp and the dropout of the normalised weights.
struct AttTrain {
    float *lse;               // [R, H, Tq]
    const long long *seed;    // one int64 on the device (read only when thresh != 0)
    unsigned thresh;          // round(p * 2^32): element kept when its hash >= thresh; 0 = no dropout
    float inv_keep;           // dropout_scale_f32(p)
};

// The dropout decision of element idx = ((r * H + h) * Tq + i) * Tk + j is dropout_keep(seed, idx, thresh) of t5_common.h.

// PACKED (no key mask, no ancestor table): a.Tq and a.Tk are the padded BOUNDS -- they keep the LDS layout, the bias
// index and the dropout element index of the padded call -- and the workgroup's own lengths Tq, Tk, read through the
// cumulative tables, give its loop bounds, its row bases and the K/V rows it stages.  A packed q has one K/V per group
// (beams = 1); a dense q over packed K/V (cu_q null) keeps the dense arm's groups of beams: rows b * beams .. of q read
// the packed group b, staged once with its own length (rqhip_t5_attention_packed_beams; beams = 1 everywhere else).
template <int MT, bool TRAIN, bool PACKED>
__device__ __forceinline__ void att_body(AttArgs a, AttTrain t) {
    extern __shared__ float att_lds[];
    const long long b = blockIdx.x / a.H;
    const int h = blockIdx.x - (int)b * a.H;
    const int tid = threadIdx.x, nthr = blockDim.x;

    int Tq = a.Tq, Tk = a.Tk;                 // this group's own lengths
    long long kbase = b * a.Tk, qbase = 0;    // first K/V row; first q / out row of a packed q
    if constexpr (PACKED) {
        if (a.cu_k) packed_group(a.cu_k, b, a.n_k, a.Tk, kbase, Tk);
        if (a.cu_q) packed_group(a.cu_q, b, a.n_q, a.Tq, qbase, Tq);
    }
    const int ntiles = (Tk + 15) >> 4, Tkp = ntiles << 4;
    const int TkpL = ((a.Tk + 15) >> 4) << 4;  // the layout's
    float *Ks = att_lds;
    float *Vs = Ks + (size_t)TkpL * kAttLd;
    float *madd = Vs + (size_t)TkpL * kAttLd;  // 0: kept, -FLT_MAX: masked, -inf: padding beyond Tk
    float *bias_s = madd + TkpL;               // [Tq + Tk - 1] of this head, by j - i + Tq - 1

    // ---- stage K, V (zeros beyond Tk: 0 * p must stay 0), the key mask and the head's bias column
    for (int idx = tid; idx < Tkp * 16; idx += nthr) {
        const int j = idx >> 4, c = idx & 15;
        float4 kk = make_float4(0.f, 0.f, 0.f, 0.f), vv = kk;
        if (j < Tk) {
            long long tok;
            if (!PACKED && a.anc) {
                long long row = b;
                if (j < a.past) {
                    row = a.anc[b * a.ld_anc + j];
                    row = row < 0 ? 0 : (row >= a.slab_rows ? a.slab_rows - 1 : row);
                }
                tok = (long long)j * a.slab_rows + row;
            } else {
                tok = kbase + j;
            }
            const size_t off = (size_t)tok * (size_t)a.ld_kv + (size_t)h * kAttD + 4 * c;
            kk = *reinterpret_cast<const float4 *>(a.k + off);
            vv = *reinterpret_cast<const float4 *>(a.v + off);
        }
        *reinterpret_cast<float4 *>(Ks + j * kAttLd + 4 * c) = kk;
        *reinterpret_cast<float4 *>(Vs + j * kAttLd + 4 * c) = vv;
    }
    for (int j = tid; j < Tkp; j += nthr)
        madd[j] = j >= Tk ? -INFINITY : ((!PACKED && a.key_mask && !a.key_mask[b * a.Tk + j]) ? -FLT_MAX : 0.f);
    if (a.bias)
        for (int x = tid; x < a.Tq + a.Tk - 1; x += nthr) bias_s[x] = a.bias[(size_t)(a.bias_base + x) * a.H + h];
    __syncthreads();

    const int nw = nthr / RQ_WAVE, wave = tid / RQ_WAVE, lane = tid & (RQ_WAVE - 1);
    const int i = lane & 15, g = lane >> 4;
    const bool qpacked = PACKED && a.cu_q;
    const int M = qpacked ? Tq : a.beams * a.Tq;
    for (int qt = wave; qt * 16 < M; qt += nw) {
        const int m = qt * 16 + i;
        const int mc = m < M ? m : M - 1;  // lanes past the last query recompute it and store nothing
        const int beam = qpacked ? 0 : mc / a.Tq, ti = mc - beam * a.Tq;
        const size_t qrow = qpacked ? (size_t)(qbase + ti) : (size_t)(b * a.beams + beam) * (size_t)a.Tq + (size_t)ti;
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
                        if (ma != 0.f || (!PACKED && a.causal && j > ti + a.past)) sc = sc + -FLT_MAX;
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
        if constexpr (PACKED) {
            if (ntiles == 0) sum = 1.f;  // a group without keys: out = 0 and lse = -inf, not 0 / 0
        }
        if constexpr (TRAIN) {
            const size_t qh = ((size_t)(b * a.beams + beam) * (size_t)a.H + (size_t)h) * (size_t)a.Tq + (size_t)ti;
            // packed q: lse is [n_q, H], a token's heads side by side
            const size_t lrow = qpacked ? qrow * (size_t)a.H + (size_t)h : qh;
            if (m < M && g == 0) t.lse[lrow] = mx + logf(sum);
            if (t.thresh) {  // dropout of the normalised weights: the dropped ones leave the product, the sum stays
                const unsigned long long seed = (unsigned long long)*t.seed;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    if (mt < ntiles) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (!dropout_keep(seed, (unsigned long long)qh * a.Tk + (16 * mt + 4 * g + r), t.thresh))
                                s[mt][r] = 0.f;
                    }
                }
            }
        }

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
            for (int dt = 0; dt < 4; ++dt) {
                if constexpr (TRAIN)  // times 1 / (1 - p), which is 1.0f at p = 0: the bits of the inference kernel
                    *reinterpret_cast<float4 *>(op + 16 * dt) =
                        make_float4(o[dt][0] / sum * t.inv_keep, o[dt][1] / sum * t.inv_keep, o[dt][2] / sum * t.inv_keep,
                                    o[dt][3] / sum * t.inv_keep);
                else
                    *reinterpret_cast<float4 *>(op + 16 * dt) =
                        make_float4(o[dt][0] / sum, o[dt][1] / sum, o[dt][2] / sum, o[dt][3] / sum);
            }
        }
    }
}

template <int MT, bool PACKED = false>
__global__ __launch_bounds__(256) void t5_attention_kernel(AttArgs a) {
    att_body<MT, false, PACKED>(a, AttTrain{});
}

template <int MT, bool PACKED = false>
__global__ __launch_bounds__(256) void t5_attention_train_kernel(AttArgs a, AttTrain t) {
    att_body<MT, true, PACKED>(a, t);
}

size_t att_lds_bytes(int Tq, int Tk, bool bias) {
    const size_t Tkp = (size_t)((Tk + 15) / 16) * 16;
    return (2 * Tkp * kAttLd + Tkp + (bias ? (size_t)(Tq + Tk - 1) : 0)) * sizeof(float);
}

// The most keys an instantiation can meet: the LDS grant is made once per device and never raised again.
constexpr int att_most_tk(int MT) { return MT * 16 < kAttMaxT ? MT * 16 : kAttMaxT; }

// One launch of any of the three attention kernels.  `most`: the dynamic LDS the grant asks for; the grant is one static
// per instantiation of this template, that is per kernel instantiation.
template <auto Kernel, class... Args>
int launch_att(const char *name, size_t most, long long blocks, int threads, size_t lds, hipStream_t s, const Args &...args) {
    if (lds > 64 * 1024) {
        static LdsGrant grant;
        RQ_RETURN_IF_HIP(grant.ensure(reinterpret_cast<const void *>(Kernel), (int)most));
    }
    hipLaunchKernelGGL(Kernel, dim3((unsigned)blocks), dim3(threads), lds, s, args...);
    RQ_CHECK_LAUNCH(name);
    return RQHIP_OK;
}

// The kernels' MT (key tiles a lane holds in registers) for Tk keys: f(std::integral_constant<int, MT>).
template <class F>
int att_with_mt(int Tk, F f) {
    const int ntiles = (Tk + 15) / 16;
    if (ntiles == 1) return f(std::integral_constant<int, 1>{});
    if (ntiles <= 6) return f(std::integral_constant<int, 6>{});
    return f(std::integral_constant<int, 16>{});
}

// ---- backward
//
// One workgroup per (row, head), two passes over one LDS buffer; P is recomputed, nothing of size Tq x Tk is stored.
//   pass 1, query-major: K and V staged as in the forward; a wave takes sixteen queries, recomputes their scores, row
//     max and row sum exactly as the forward did (the bits of its P), then
//       dP^T = V dO^T (o M / (1 - p)), D_i = sum_j P_ij dP_ij (= dO_i . O_i), dS = P o (dP - D), dQ^T += K^T dS^T
//     in the forward's register layout (lane (g, i) holds keys 16 mt + 4 g + r of query i), and leaves max, sum and D
//     of its queries in LDS.
//   pass 2, key-major: Q and dO staged in the same buffer; a wave takes sixteen keys (K and V rows in registers) and
//     loops over the query tiles, S = Q K^T and dP = dO V^T now with lane (g, c) holding queries 16 qt + 4 g + r of key
//     c, and accumulates dK^T += Q^T dS, dV^T += dO^T (P o M / (1 - p)) in registers.
//   bias gradient: the sums of dS along the diagonals j - i.  Pass 1 puts each 16 x 16 tile of dS through a per-wave LDS
//     scratch, lane d < 31 adds diagonal d - 15 (queries ascending) into the wave's own [Tq + Tk - 1] row; the waves'
//     rows are added in wave order into d_bias_partial[(r, h)], and t5_dbias_reduce_kernel adds the rows r in order.
// The row's normaliser comes from pass 1, not from lse: max + log(sum) rounds log(sum) away when every key of a row is
// masked (max = -FLT_MAX), and that row's P must still be uniform.  Nor is `out` read: D comes from P and dP (above).
struct AttBwdArgs {
    const float *q, *k, *v, *d_out;
    float *dq, *dk, *dv, *dbias_part;
    long long ld_q, ld_kv, ld_do;
    int H, Tq, Tk, causal;
    const float *bias;
    int bias_base;
    const unsigned char *key_mask;
    const long long *seed;
    unsigned thresh;
    float inv_keep;
    const int *cu_q, *cu_k;  // as in AttArgs (the packed kernels)
    long long n_q, n_k;
};

constexpr int kAttTileLd = 17;  // row stride of the per-wave 16 x 16 dS scratch

struct AttBwdLds {
    size_t big, madd, bias, mx, sum, dd, dbw, tile, total;  // offsets in floats
};

__host__ __device__ inline AttBwdLds att_bwd_lds(int Tq, int Tk, bool bias, int nw) {
    const size_t Tqp = (size_t)((Tq + 15) / 16) * 16, Tkp = (size_t)((Tk + 15) / 16) * 16;
    const size_t Tp = Tqp > Tkp ? Tqp : Tkp, nb = bias ? (size_t)(Tq + Tk - 1) : 0;
    AttBwdLds l;
    l.big = 0;
    l.madd = 2 * Tp * kAttLd;
    l.bias = l.madd + Tkp;
    l.mx = l.bias + nb;
    l.sum = l.mx + Tqp;
    l.dd = l.sum + Tqp;
    l.dbw = l.dd + Tqp;
    l.tile = l.dbw + (size_t)nw * nb;
    l.total = l.tile + (bias ? (size_t)nw * 16 * kAttTileLd : 0);
    return l;
}

// PACKED: as in att_body -- a.Tq and a.Tk are the padded bounds (LDS layout, bias index, the partial row's width and
// the dropout element index), Tq and Tk the workgroup's own lengths.
template <int MT, bool PACKED = false>
__global__ __launch_bounds__(256) void t5_attention_bwd_kernel(AttBwdArgs a) {
    extern __shared__ float att_lds[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int nw = nthr / RQ_WAVE, wave = tid / RQ_WAVE, lane = tid & (RQ_WAVE - 1);
    const int i = lane & 15, g = lane >> 4;
    const long long b = blockIdx.x / a.H;
    const int h = blockIdx.x - (int)b * a.H;
    int Tq = a.Tq, Tk = a.Tk;                          // this group's own lengths
    long long kbase = b * a.Tk, qbase = b * a.Tq;      // first K/V row, first q / d_out / dq row
    if constexpr (PACKED) {
        if (a.cu_k) packed_group(a.cu_k, b, a.n_k, a.Tk, kbase, Tk);
        if (a.cu_q) packed_group(a.cu_q, b, a.n_q, a.Tq, qbase, Tq);
    }
    const int ntiles = (Tk + 15) >> 4, Tkp = ntiles << 4, Tqp = ((Tq + 15) >> 4) << 4;
    const int nb = a.bias ? a.Tq + a.Tk - 1 : 0;
    const AttBwdLds L = att_bwd_lds(a.Tq, a.Tk, a.bias != nullptr, nw);
    float *Ks = att_lds, *Vs = Ks + L.madd / 2;  // two buffers of max(Tqp, Tkp) padded rows; pass 2: Q and dO
    float *madd = att_lds + L.madd, *bias_s = att_lds + L.bias;
    float *mx_s = att_lds + L.mx, *sum_s = att_lds + L.sum, *dd_s = att_lds + L.dd;
    float *dbw = att_lds + L.dbw + (size_t)wave * nb, *tile = att_lds + L.tile + (size_t)wave * 16 * kAttTileLd;

    const unsigned long long seed = a.thresh ? (unsigned long long)*a.seed : 0ull;
    const unsigned long long idx0 = ((unsigned long long)b * a.H + h) * (unsigned long long)a.Tq;  // + i, then * Tk + j

    // ---- pass 1: stage K, V (zeros beyond Tk), the key mask, the head's bias column; clear the waves' bias rows
    for (int idx = tid; idx < Tkp * 16; idx += nthr) {
        const int j = idx >> 4, c = idx & 15;
        float4 kk = make_float4(0.f, 0.f, 0.f, 0.f), vv = kk;
        if (j < Tk) {
            const size_t off = (size_t)(kbase + j) * (size_t)a.ld_kv + (size_t)h * kAttD + 4 * c;
            kk = *reinterpret_cast<const float4 *>(a.k + off);
            vv = *reinterpret_cast<const float4 *>(a.v + off);
        }
        *reinterpret_cast<float4 *>(Ks + j * kAttLd + 4 * c) = kk;
        *reinterpret_cast<float4 *>(Vs + j * kAttLd + 4 * c) = vv;
    }
    for (int j = tid; j < Tkp; j += nthr)
        madd[j] = j >= Tk ? -INFINITY : ((!PACKED && a.key_mask && !a.key_mask[b * a.Tk + j]) ? -FLT_MAX : 0.f);
    for (int x = tid; x < nb; x += nthr) bias_s[x] = a.bias[(size_t)(a.bias_base + x) * a.H + h];
    for (int x = tid; x < nw * nb; x += nthr) att_lds[L.dbw + x] = 0.f;
    __syncthreads();

    for (int qt = wave; qt * 16 < Tq; qt += nw) {
        const int m = qt * 16 + i;
        const int ti = m < Tq ? m : Tq - 1;  // lanes past the last query recompute it and contribute nothing
        const size_t qrow = (size_t)(qbase + ti);
        const float *qp = a.q + qrow * (size_t)a.ld_q + (size_t)h * kAttD + g;
        const float *dop = a.d_out + qrow * (size_t)a.ld_do + (size_t)h * kAttD + g;
        float qreg[16], doreg[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) qreg[e] = qp[4 * e], doreg[e] = dop[4 * e];

        // ---- scores, bias, masks, row max and row sum: the forward's sequence
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
                        if (ma != 0.f || (!PACKED && a.causal && j > ti)) sc = sc + -FLT_MAX;
                    }
                    s[mt][r] = sc;
                    mx = fmaxf(mx, sc);
                }
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, RQ_WAVE));
        mx = fmaxf(mx, __shfl_xor(mx, 32, RQ_WAVE));
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

        // ---- dP = (dO V^T) o M / (1 - p) of the whole row, and D = sum_j P dP (the lane's keys in order, then the four
        // lanes of the query).  D is dO . O, evaluated from the dP that dS subtracts it from: the rounding of the 64-term
        // products then cancels in dP - D as it does in the operators' softmax backward, and a row with one live key
        // (P = 1, the others exactly 0) has D = dP and dS = 0 exactly.
        f32x4 dp[MT];
        float D = 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            dp[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (mt < ntiles) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                const float *vp = Vs + (16 * mt + i) * kAttLd + g;
#pragma unroll
                for (int e = 0; e < 16; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[4 * e], doreg[e], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float d = acc[r];
                    if (a.thresh)
                        d = dropout_keep(seed, (idx0 + ti) * a.Tk + (16 * mt + 4 * g + r), a.thresh) ? d * a.inv_keep : 0.f;
                    const float p = s[mt][r] / sum;
                    s[mt][r] = p;
                    dp[mt][r] = d;
                    D = D + p * d;
                }
            }
        }
        D = D + __shfl_xor(D, 16, RQ_WAVE);
        D = D + __shfl_xor(D, 32, RQ_WAVE);
        if (m < Tq && g == 0) mx_s[m] = mx, sum_s[m] = sum, dd_s[m] = D;

        // ---- per key tile: dS, the tile's diagonal sums, dQ
        f32x4 dq[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (mt < ntiles) {
                f32x4 ds;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float d = s[mt][r] * (dp[mt][r] - D);
                    ds[r] = m < Tq ? d : 0.f;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float *kp = Ks + (16 * mt + 4 * g + r) * kAttLd + i;
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt)
                        dq[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kp[16 * dt], ds[r], dq[dt], 0, 0, 0);
                }
                if (a.bias) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) tile[i * kAttTileLd + 4 * g + r] = ds[r];
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the scratch and the row are this wave's only
                    if (lane < 31) {
                        const int dl = lane - 15;  // key - query inside the tile
                        const int lo = dl < 0 ? -dl : 0, hi = dl > 0 ? 15 - dl : 15;
                        float acc1 = 0.f;
                        for (int ii = lo; ii <= hi; ++ii) acc1 = acc1 + tile[ii * kAttTileLd + ii + dl];
                        const int x = 16 * (mt - qt) + dl + a.Tq - 1;
                        if (x >= 0 && x < nb) dbw[x] = dbw[x] + acc1;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                }
            }
        }
        if (m < Tq) {
            float *dqp = a.dq + qrow * (size_t)a.H * kAttD + (size_t)h * kAttD + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<float4 *>(dqp + 16 * dt) = make_float4(dq[dt][0], dq[dt][1], dq[dt][2], dq[dt][3]);
        }
    }
    __syncthreads();

    // ---- the waves' bias rows in wave order; then Q and dO take the place of K and V (zeros beyond Tq)
    for (int x = tid; x < nb; x += nthr) {
        float acc1 = att_lds[L.dbw + x];
        for (int w = 1; w < nw; ++w) acc1 = acc1 + att_lds[L.dbw + (size_t)w * nb + x];
        a.dbias_part[(size_t)blockIdx.x * nb + x] = acc1;
    }
    float *Qs = Ks, *dOs = Vs;
    for (int idx = tid; idx < Tqp * 16; idx += nthr) {
        const int ii = idx >> 4, c = idx & 15;
        float4 qq = make_float4(0.f, 0.f, 0.f, 0.f), dd = qq;
        if (ii < Tq) {
            const size_t row = (size_t)(qbase + ii);
            qq = *reinterpret_cast<const float4 *>(a.q + row * (size_t)a.ld_q + (size_t)h * kAttD + 4 * c);
            dd = *reinterpret_cast<const float4 *>(a.d_out + row * (size_t)a.ld_do + (size_t)h * kAttD + 4 * c);
        }
        *reinterpret_cast<float4 *>(Qs + ii * kAttLd + 4 * c) = qq;
        *reinterpret_cast<float4 *>(dOs + ii * kAttLd + 4 * c) = dd;
    }
    __syncthreads();

    // ---- pass 2: lane (g, c) owns key 16 kt + c and, per query tile, queries 16 qt + 4 g + r
    for (int kt = wave; kt * 16 < Tk; kt += nw) {
        const int j = kt * 16 + i;
        const int jc = j < Tk ? j : Tk - 1;
        const size_t krow = (size_t)(kbase + jc);
        const float *kp = a.k + krow * (size_t)a.ld_kv + (size_t)h * kAttD + g;
        const float *vp = a.v + krow * (size_t)a.ld_kv + (size_t)h * kAttD + g;
        float kreg[16], vreg[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) kreg[e] = kp[4 * e], vreg[e] = vp[4 * e];
        const float ma = madd[kt * 16 + i];
        f32x4 dk[4], dv[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dk[dt] = dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int qt = 0; qt * 16 < Tq; ++qt) {
            f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, pacc = sacc;
            const float *qs = Qs + (16 * qt + i) * kAttLd + g, *dos = dOs + (16 * qt + i) * kAttLd + g;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                sacc = __builtin_amdgcn_mfma_f32_16x16x4f32(qs[4 * e], kreg[e], sacc, 0, 0, 0);
                pacc = __builtin_amdgcn_mfma_f32_16x16x4f32(dos[4 * e], vreg[e], pacc, 0, 0, 0);
            }
            f32x4 ds, pd;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qi = 16 * qt + 4 * g + r;
                const int ti = qi < Tq ? qi : Tq - 1;
                float sc = sacc[r];
                if (a.bias) sc = sc + bias_s[jc - ti + a.Tq - 1];
                if (ma != 0.f || (!PACKED && a.causal && j > ti)) sc = sc + -FLT_MAX;
                float p = expf(sc - mx_s[ti]) / sum_s[ti];
                if (qi >= Tq || j >= Tk) p = 0.f;
                float dp = pacc[r], pk = p;
                if (a.thresh) {
                    const bool keep = dropout_keep(seed, (idx0 + ti) * a.Tk + jc, a.thresh);
                    dp = keep ? dp * a.inv_keep : 0.f;
                    pk = keep ? p * a.inv_keep : 0.f;
                }
                ds[r] = p * (dp - dd_s[ti]);
                pd[r] = pk;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float *q2 = Qs + (16 * qt + 4 * g + r) * kAttLd + i, *do2 = dOs + (16 * qt + 4 * g + r) * kAttLd + i;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    dk[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(q2[16 * dt], ds[r], dk[dt], 0, 0, 0);
                    dv[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(do2[16 * dt], pd[r], dv[dt], 0, 0, 0);
                }
            }
        }
        if (j < Tk) {
            const size_t off = krow * (size_t)a.H * kAttD + (size_t)h * kAttD + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                *reinterpret_cast<float4 *>(a.dk + off + 16 * dt) = make_float4(dk[dt][0], dk[dt][1], dk[dt][2], dk[dt][3]);
                *reinterpret_cast<float4 *>(a.dv + off + 16 * dt) = make_float4(dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]);
            }
        }
    }
}

// d_bias[row, h] = sum over the rows r, ascending, of part[(r, h)][row - base]; zero outside the call's delta range.
__global__ __launch_bounds__(256) void t5_dbias_reduce_kernel(const float *part, long long R, int H, int nb, int base,
                                                              int n_delta, float *out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n_delta * H) return;
    const int row = (int)(idx / H), h = (int)(idx - (long long)row * H);
    float acc = 0.f;
    if (row >= base && row < base + nb)
        for (long long r = 0; r < R; ++r) acc = acc + part[((size_t)r * H + h) * (size_t)nb + (row - base)];
    out[idx] = acc;
}

bool att_supported(int d_kv, int H, int Tq, int Tk) {
    return d_kv == kAttD && H >= 1 && Tq >= 1 && Tq <= kAttMaxT && Tk >= 1 && Tk <= kAttMaxT;
}

// The checks the three entry points share, in their one order; `who` names the entry point in the message.  The
// inference call passes its `past` and ancestor table (and p = 0); the training pair (`train`) passes 0 / null, takes
// one K/V per row and has no group of beams.  `strides`: the call's row strides, q, k/v and out first.
int check_att_call(const char *who, bool train, int64_t R, int64_t Rk, int H, int d_kv, int Tq, int Tk, int past,
                   const int32_t *anc, int64_t ld_anc, int64_t slab_rows, std::initializer_list<int64_t> strides,
                   const float *bias, int n_delta, int bias_offset, int causal, double p) {
    if (R < 0 || Rk < 0 || H < 1 || d_kv < 1 || Tq < 1 || Tk < 1 || past < 0) {
        set_error("%s: bad sizes (R=%lld, Rk=%lld, H=%d, d_kv=%d, Tq=%d, Tk=%d, past=%d)", who, (long long)R,
                  (long long)Rk, H, d_kv, Tq, Tk, past);
        return RQHIP_EARG;
    }
    if (d_kv != kAttD) {
        set_error("%s: d_kv=%d, only d_kv = %d is implemented", who, d_kv, kAttD);
        return RQHIP_EUNSUPPORTED;
    }
    if (Tq > kAttMaxT || Tk > kAttMaxT) {
        set_error("%s: Tq=%d / Tk=%d exceed Tq, Tk <= %d", who, Tq, Tk, kAttMaxT);
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
    const int64_t inner = (int64_t)H * kAttD;
    bool strides_ok = true;
    for (const int64_t ld : strides) strides_ok = strides_ok && ld >= inner && ld % 4 == 0;
    if (!strides_ok) {
        if (train)
            set_error("%s: row strides must be multiples of 4 and >= H * 64 = %lld", who, (long long)inner);
        else
            set_error("%s: row strides (q %lld, k/v %lld, out %lld) must be multiples of 4 and >= H * 64 = %lld", who,
                      (long long)strides.begin()[0], (long long)strides.begin()[1], (long long)strides.begin()[2],
                      (long long)inner);
        return RQHIP_EARG;
    }
    if (anc) {
        if (Tq != 1 || Rk != R || Tk != past + 1 || ld_anc < past || slab_rows < R) {
            set_error("%s: the ancestor table takes Tq = 1, Rk = R, Tk = past + 1, ld_anc >= past and "
                      "slab_rows >= R (Tq=%d, R=%lld, Rk=%lld, Tk=%d, past=%d, ld_anc=%lld, slab_rows=%lld)",
                      who, Tq, (long long)R, (long long)Rk, Tk, past, (long long)ld_anc, (long long)slab_rows);
            return RQHIP_EARG;
        }
    } else if (past + Tq > Tk && (causal || bias)) {
        if (train)
            set_error("%s: Tq = %d exceeds Tk = %d", who, Tq, Tk);
        else
            set_error("%s: past + Tq = %d exceeds Tk = %d", who, past + Tq, Tk);
        return RQHIP_EARG;
    }
    const int bias_base = bias_offset - (Tq - 1) - past;
    if (bias && (bias_base < 0 || (int64_t)bias_base + Tq + Tk - 1 > n_delta)) {
        set_error("%s: the bias table (n_delta=%d, offset=%d) does not cover deltas %d .. %d", who, n_delta, bias_offset,
                  -(Tq - 1) - past, Tk - 1 - past);
        return RQHIP_EARG;
    }
    if (!dropout_p_valid(p)) {
        set_error("%s: dropout probability p=%g outside 0 <= p < 1", who, p);
        return RQHIP_EARG;
    }
    if (Rk * (int64_t)H >= (1ll << 31)) {
        if (train)
            set_error("%s: R * H = %lld exceeds one workgroup per (row, head) (< 2^31)", who, (long long)(Rk * (int64_t)H));
        else
            set_error("%s: Rk * H = %lld exceeds one workgroup per (group, head) (< 2^31)", who,
                      (long long)(Rk * (int64_t)H));
        return RQHIP_EUNSUPPORTED;
    }
    return RQHIP_OK;
}

// The packed form of a call: the cumulative row tables and row counts the PACKED kernels read, and the key_mask / causal
// the caller passed, which check_packed_call rejects.  A null descriptor is the padded form.
struct AttPacked {
    const int32_t *cu_q, *cu_k;
    int64_t n_q, n_k;
    const uint8_t *key_mask;
    int causal;
    bool beams = false;  // rqhip_t5_attention_packed_beams: dense q in groups of R / Rk rows over Rk packed K/V groups
};

// What the packed entry points check beyond check_att_call: the tables and the row counts they index (R groups of
// queries, Rk of keys: the same number everywhere but in the beams call).
int check_packed_call(const char *who, int64_t R, int64_t Rk, int Tq, int Tk, const AttPacked &pk) {
    if (pk.beams) {
        if (!pk.cu_k) {
            set_error("%s: cu_k is null: the K/V groups are packed behind their cumulative table", who);
            return RQHIP_EARG;
        }
        if (pk.n_k < 0 || pk.n_k >= (1ll << 31) || pk.n_k > Rk * Tk) {
            set_error("%s: n_k=%lld rows do not go with Rk=%lld groups of at most Tk=%d (int32 table)", who,
                      (long long)pk.n_k, (long long)Rk, Tk);
            return RQHIP_EARG;
        }
        return RQHIP_OK;
    }
    if (!pk.cu_q && !pk.cu_k) {
        set_error("%s: no cumulative table (cu_q, cu_k): the dense call is rqhip_t5_attention*", who);
        return RQHIP_EARG;
    }
    if (pk.causal || pk.key_mask) {
        set_error("%s: a cumulative table goes with neither causal nor key_mask (every packed key is valid)", who);
        return RQHIP_EARG;
    }
    if (pk.n_q < 0 || pk.n_k < 0 || pk.n_q >= (1ll << 31) || pk.n_k >= (1ll << 31) || (!pk.cu_q && pk.n_q != R * Tq) ||
        (!pk.cu_k && pk.n_k != R * Tk) || pk.n_q > R * Tq || pk.n_k > R * Tk) {
        set_error("%s: n_q=%lld / n_k=%lld rows do not go with R=%lld groups of at most Tq=%d / Tk=%d (a dense side "
                  "holds exactly R * T rows; int32 tables)", who, (long long)pk.n_q, (long long)pk.n_k, (long long)R, Tq, Tk);
        return RQHIP_EARG;
    }
    return RQHIP_OK;
}

// ---- the three calls behind the seven entry points: checks, null and alignment tests, struct fill and launch, each once.
// `pk`: the packed form, which runs the same kernel bodies in their PACKED instantiations (lengths per group through
// cu_q / cu_k, the padded call's plan by the bounds).  Its entry points pass Rk = R and key_mask = null, causal = 0 (the
// caller's are in *pk), and it is checked as the training pair is: one K/V per row -- but for the beams call, which
// passes its own Rk and is checked as the dense inference call is.

int att_fwd_call(const char *who, const AttPacked *pk, const float *q, int64_t ld_q, const float *k, const float *v,
                 int64_t ld_kv, int64_t R, int64_t Rk, int H, int d_kv, int Tq, int Tk, const float *bias_by_delta,
                 int n_delta, int bias_offset, const uint8_t *key_mask, int causal, int past, const int32_t *anc,
                 int64_t ld_anc, int64_t slab_rows, float *out, int64_t ld_out, rqhip_stream_t stream) {
    int rc = check_att_call(who, pk && !pk->beams, R, Rk, H, d_kv, Tq, Tk, past, anc, ld_anc, slab_rows,
                            {ld_q, ld_kv, ld_out}, bias_by_delta, n_delta, bias_offset, causal, 0.0);
    if (rc == RQHIP_OK && pk) rc = check_packed_call(who, R, Rk, Tq, Tk, *pk);
    if (rc != RQHIP_OK) return rc;
    if (R == 0 || (pk && pk->n_q == 0)) return RQHIP_OK;
    if (any_null(q, out) || ((!pk || pk->n_k > 0) && any_null(k, v))) {
        set_error("%s: null pointer (q, k, v, out)", who);
        return RQHIP_EARG;
    }
    if (!all_aligned16(q, k, v, out)) {
        set_error("%s: q, k, v and out must be 16-byte aligned", who);
        return RQHIP_EARG;
    }
    const AttPacked form = pk ? *pk : AttPacked{};
    AttArgs a;
    a.q = q, a.k = k, a.v = v, a.out = out;
    a.ld_q = ld_q, a.ld_kv = ld_kv, a.ld_out = ld_out;
    a.beams = (int)(R / Rk), a.H = H, a.Tq = Tq, a.Tk = Tk, a.past = past, a.causal = causal != 0;
    a.bias = bias_by_delta, a.bias_base = bias_offset - (Tq - 1) - past;  // table row of the smallest delta j - i - past
    a.key_mask = key_mask;
    a.anc = past > 0 ? anc : nullptr;  // at past = 0 the only key is the row's own: the dense form of slab 0
    a.ld_anc = ld_anc, a.slab_rows = slab_rows;
    a.cu_q = form.cu_q, a.cu_k = form.cu_k, a.n_q = form.n_q, a.n_k = form.n_k;
    if ((int64_t)a.beams * Tq >= (1ll << 24)) {
        set_error("%s: %lld query rows per K/V group", who, (long long)a.beams * Tq);
        return RQHIP_EUNSUPPORTED;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = att_lds_bytes(Tq, Tk, bias_by_delta != nullptr);
    return att_with_mt(Tk, [&](auto mt) {
        constexpr int MT = decltype(mt)::value;
        const size_t most = att_lds_bytes(kAttMaxT, att_most_tk(MT), true);
        const int threads = MT == 1 ? RQ_WAVE : 4 * RQ_WAVE;
        return pk ? launch_att<t5_attention_kernel<MT, true>>("t5_attention_kernel (packed)", most, Rk * H, threads, lds, s,
                                                              a)
                  : launch_att<t5_attention_kernel<MT, false>>("t5_attention_kernel", most, Rk * H, threads, lds, s, a);
    });
}

int att_fwd_train_call(const char *who, const AttPacked *pk, const float *q, int64_t ld_q, const float *k, const float *v,
                       int64_t ld_kv, int64_t R, int64_t Rk, int H, int d_kv, int Tq, int Tk, const float *bias_by_delta,
                       int n_delta, int bias_offset, const uint8_t *key_mask, int causal, double p, const int64_t *seed,
                       float *out, int64_t ld_out, float *lse, rqhip_stream_t stream) {
    int rc = check_att_call(who, true, R, Rk, H, d_kv, Tq, Tk, 0, nullptr, 0, 0, {ld_q, ld_kv, ld_out}, bias_by_delta,
                            n_delta, bias_offset, causal, p);
    if (rc == RQHIP_OK && pk) rc = check_packed_call(who, R, R, Tq, Tk, *pk);
    if (rc != RQHIP_OK) return rc;
    if (R == 0 || (pk && pk->n_q == 0)) return RQHIP_OK;
    const unsigned thresh = dropout_threshold(p);
    if (any_null(q, out, lse) || ((!pk || pk->n_k > 0) && any_null(k, v)) || (thresh && !seed)) {
        set_error("%s: null pointer (q, k, v, out, lse; seed when p > 0)", who);
        return RQHIP_EARG;
    }
    if (!all_aligned16(q, k, v, out)) {
        set_error("%s: q, k, v and out must be 16-byte aligned", who);
        return RQHIP_EARG;
    }
    const AttPacked form = pk ? *pk : AttPacked{};
    AttArgs a;
    a.q = q, a.k = k, a.v = v, a.out = out;
    a.ld_q = ld_q, a.ld_kv = ld_kv, a.ld_out = ld_out;
    a.beams = 1, a.H = H, a.Tq = Tq, a.Tk = Tk, a.past = 0, a.causal = causal != 0;
    a.bias = bias_by_delta, a.bias_base = bias_offset - (Tq - 1);
    a.key_mask = key_mask;
    a.anc = nullptr, a.ld_anc = 0, a.slab_rows = 0;
    a.cu_q = form.cu_q, a.cu_k = form.cu_k, a.n_q = form.n_q, a.n_k = form.n_k;
    AttTrain t;
    t.lse = lse, t.seed = reinterpret_cast<const long long *>(seed), t.thresh = thresh;
    t.inv_keep = dropout_scale_f32(p);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = att_lds_bytes(Tq, Tk, bias_by_delta != nullptr);
    return att_with_mt(Tk, [&](auto mt) {  // the inference call's plan
        constexpr int MT = decltype(mt)::value;
        const size_t most = att_lds_bytes(kAttMaxT, att_most_tk(MT), true);
        const int threads = MT == 1 ? RQ_WAVE : 4 * RQ_WAVE;
        return pk ? launch_att<t5_attention_train_kernel<MT, true>>("t5_attention_train_kernel (packed)", most, R * H,
                                                                    threads, lds, s, a, t)
                  : launch_att<t5_attention_train_kernel<MT, false>>("t5_attention_train_kernel", most, R * H, threads,
                                                                     lds, s, a, t);
    });
}

int att_bwd_call(const char *who, const AttPacked *pk, const float *q, int64_t ld_q, const float *k, const float *v,
                 int64_t ld_kv, const float *out, int64_t ld_out, const float *lse, const float *d_out, int64_t ld_do,
                 int64_t R, int64_t Rk, int H, int d_kv, int Tq, int Tk, const float *bias_by_delta, int n_delta,
                 int bias_offset, const uint8_t *key_mask, int causal, double p, const int64_t *seed, float *d_q,
                 float *d_k, float *d_v, float *d_bias_by_delta, float *d_bias_partial, rqhip_stream_t stream) {
    int rc = check_att_call(who, true, R, Rk, H, d_kv, Tq, Tk, 0, nullptr, 0, 0, {ld_q, ld_kv, ld_out, ld_do}, bias_by_delta,
                            n_delta, bias_offset, causal, p);
    if (rc == RQHIP_OK && pk) rc = check_packed_call(who, R, R, Tq, Tk, *pk);
    if (rc != RQHIP_OK) return rc;
    if (R == 0 && !bias_by_delta) return RQHIP_OK;
    const unsigned thresh = dropout_threshold(p);
    // a packed side without rows may be null
    if (((!pk || pk->n_q > 0) && any_null(q, out, lse, d_out, d_q)) || ((!pk || pk->n_k > 0) && any_null(k, v, d_k, d_v)) ||
        (thresh && !seed) || (bias_by_delta && any_null(d_bias_by_delta, d_bias_partial))) {
        set_error("%s: null pointer (q, k, v, out, lse, d_out, d_q, d_k, d_v; seed when p > 0; "
                  "d_bias_by_delta and d_bias_partial with a bias table)", who);
        return RQHIP_EARG;
    }
    if (!all_aligned16(q, k, v, out, d_out, d_q, d_k, d_v)) {
        set_error("%s: q, k, v, out, d_out, d_q, d_k and d_v must be 16-byte aligned", who);
        return RQHIP_EARG;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nb = Tq + Tk - 1;
    if (R > 0) {
        const AttPacked form = pk ? *pk : AttPacked{};
        AttBwdArgs a;
        a.q = q, a.k = k, a.v = v, a.d_out = d_out;
        a.dq = d_q, a.dk = d_k, a.dv = d_v, a.dbias_part = d_bias_partial;
        a.ld_q = ld_q, a.ld_kv = ld_kv, a.ld_do = ld_do;
        a.H = H, a.Tq = Tq, a.Tk = Tk, a.causal = causal != 0;
        a.bias = bias_by_delta, a.bias_base = bias_offset - (Tq - 1);
        a.key_mask = key_mask;
        a.seed = reinterpret_cast<const long long *>(seed), a.thresh = thresh;
        a.inv_keep = dropout_scale_f32(p);
        a.cu_q = form.cu_q, a.cu_k = form.cu_k, a.n_q = form.n_q, a.n_k = form.n_k;
        const int threads = (Tq <= 16 && Tk <= 16) ? RQ_WAVE : 4 * RQ_WAVE;
        const size_t lds = att_bwd_lds(Tq, Tk, bias_by_delta != nullptr, threads / RQ_WAVE).total * sizeof(float);
        const int lrc = att_with_mt(Tk, [&](auto mt) {
            constexpr int MT = decltype(mt)::value;
            const size_t most = att_bwd_lds(kAttMaxT, att_most_tk(MT), true, 4).total * sizeof(float);
            return pk ? launch_att<t5_attention_bwd_kernel<MT, true>>("t5_attention_bwd_kernel (packed)", most, R * H,
                                                                      threads, lds, s, a)
                      : launch_att<t5_attention_bwd_kernel<MT, false>>("t5_attention_bwd_kernel", most, R * H, threads, lds,
                                                                       s, a);
        });
        if (lrc != RQHIP_OK) return lrc;
    }
    if (bias_by_delta) {
        const long long n = (long long)n_delta * H;
        hipLaunchKernelGGL(t5_dbias_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_bias_partial, R, H,
                           nb, bias_offset - (Tq - 1), n_delta, d_bias_by_delta);
        RQ_CHECK_LAUNCH("t5_dbias_reduce_kernel");
    }
    return RQHIP_OK;
}

}  // namespace

}  // namespace rqhip

using namespace rqhip;

extern "C" int rqhip_t5_attention_supported(int d_kv, int H, int Tq, int Tk) { return att_supported(d_kv, H, Tq, Tk); }

extern "C" int rqhip_t5_attention_bwd_supported(int d_kv, int H, int Tq, int Tk) {
    return att_supported(d_kv, H, Tq, Tk);
}

extern "C" int rqhip_t5_attention_packed_supported(int d_kv, int H, int Tq, int Tk) {
    return att_supported(d_kv, H, Tq, Tk);
}

extern "C" int rqhip_t5_attention(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, int64_t R,
                                  int64_t Rk, int H, int d_kv, int Tq, int Tk, const float *bias_by_delta, int n_delta,
                                  int bias_offset, const uint8_t *key_mask, int causal, int past, const int32_t *anc,
                                  int64_t ld_anc, int64_t slab_rows, float *out, int64_t ld_out,
                                  rqhip_stream_t stream) {
    return att_fwd_call("t5_attention", nullptr, q, ld_q, k, v, ld_kv, R, Rk, H, d_kv, Tq, Tk, bias_by_delta, n_delta,
                        bias_offset, key_mask, causal, past, anc, ld_anc, slab_rows, out, ld_out, stream);
}

extern "C" int rqhip_t5_attention_packed(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv,
                                         int64_t R, int64_t n_q, int64_t n_k, int H, int d_kv, int Tq, int Tk,
                                         const int32_t *cu_q, const int32_t *cu_k, const float *bias_by_delta,
                                         int n_delta, int bias_offset, const uint8_t *key_mask, int causal, float *out,
                                         int64_t ld_out, rqhip_stream_t stream) {
    const AttPacked pk{cu_q, cu_k, n_q, n_k, key_mask, causal};
    return att_fwd_call("t5_attention_packed", &pk, q, ld_q, k, v, ld_kv, R, R, H, d_kv, Tq, Tk, bias_by_delta, n_delta,
                        bias_offset, nullptr, 0, 0, nullptr, 0, 0, out, ld_out, stream);
}

extern "C" int rqhip_t5_attention_packed_beams(const float *q, int64_t ld_q, const float *k, const float *v,
                                               int64_t ld_kv, int64_t R, int64_t Rk, int64_t n_k, int H, int d_kv, int Tq,
                                               int Tk, const int32_t *cu_k, float *out, int64_t ld_out,
                                               rqhip_stream_t stream) {
    AttPacked pk{nullptr, cu_k, R * (int64_t)Tq, n_k, nullptr, 0};
    pk.beams = true;
    return att_fwd_call("t5_attention_packed_beams", &pk, q, ld_q, k, v, ld_kv, R, Rk, H, d_kv, Tq, Tk, nullptr, 0, 0,
                        nullptr, 0, 0, nullptr, 0, 0, out, ld_out, stream);
}

extern "C" int rqhip_t5_attention_fwd_train(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv,
                                            int64_t R, int64_t Rk, int H, int d_kv, int Tq, int Tk,
                                            const float *bias_by_delta, int n_delta, int bias_offset,
                                            const uint8_t *key_mask, int causal, double p, const int64_t *seed, float *out,
                                            int64_t ld_out, float *lse, rqhip_stream_t stream) {
    return att_fwd_train_call("t5_attention_fwd_train", nullptr, q, ld_q, k, v, ld_kv, R, Rk, H, d_kv, Tq, Tk, bias_by_delta,
                              n_delta, bias_offset, key_mask, causal, p, seed, out, ld_out, lse, stream);
}

extern "C" int rqhip_t5_attention_packed_fwd_train(const float *q, int64_t ld_q, const float *k, const float *v,
                                                   int64_t ld_kv, int64_t R, int64_t n_q, int64_t n_k, int H, int d_kv,
                                                   int Tq, int Tk, const int32_t *cu_q, const int32_t *cu_k,
                                                   const float *bias_by_delta, int n_delta, int bias_offset,
                                                   const uint8_t *key_mask, int causal, double p, const int64_t *seed,
                                                   float *out, int64_t ld_out, float *lse, rqhip_stream_t stream) {
    const AttPacked pk{cu_q, cu_k, n_q, n_k, key_mask, causal};
    return att_fwd_train_call("t5_attention_packed_fwd_train", &pk, q, ld_q, k, v, ld_kv, R, R, H, d_kv, Tq, Tk,
                              bias_by_delta, n_delta, bias_offset, nullptr, 0, p, seed, out, ld_out, lse, stream);
}

extern "C" int rqhip_t5_attention_bwd(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv,
                                      const float *out, int64_t ld_out, const float *lse, const float *d_out,
                                      int64_t ld_do, int64_t R, int64_t Rk, int H, int d_kv, int Tq, int Tk,
                                      const float *bias_by_delta, int n_delta, int bias_offset, const uint8_t *key_mask,
                                      int causal, double p, const int64_t *seed, float *d_q, float *d_k, float *d_v,
                                      float *d_bias_by_delta, float *d_bias_partial, rqhip_stream_t stream) {
    return att_bwd_call("t5_attention_bwd", nullptr, q, ld_q, k, v, ld_kv, out, ld_out, lse, d_out, ld_do, R, Rk, H, d_kv,
                        Tq, Tk, bias_by_delta, n_delta, bias_offset, key_mask, causal, p, seed, d_q, d_k, d_v,
                        d_bias_by_delta, d_bias_partial, stream);
}

extern "C" int rqhip_t5_attention_packed_bwd(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv,
                                             const float *out, int64_t ld_out, const float *lse, const float *d_out,
                                             int64_t ld_do, int64_t R, int64_t n_q, int64_t n_k, int H, int d_kv, int Tq,
                                             int Tk, const int32_t *cu_q, const int32_t *cu_k,
                                             const float *bias_by_delta, int n_delta, int bias_offset,
                                             const uint8_t *key_mask, int causal, double p, const int64_t *seed,
                                             float *d_q, float *d_k, float *d_v, float *d_bias_by_delta,
                                             float *d_bias_partial, rqhip_stream_t stream) {
    const AttPacked pk{cu_q, cu_k, n_q, n_k, key_mask, causal};
    return att_bwd_call("t5_attention_packed_bwd", &pk, q, ld_q, k, v, ld_kv, out, ld_out, lse, d_out, ld_do, R, R, H, d_kv,
                        Tq, Tk, bias_by_delta, n_delta, bias_offset, nullptr, 0, p, seed, d_q, d_k, d_v, d_bias_by_delta,
                        d_bias_partial, stream);
}

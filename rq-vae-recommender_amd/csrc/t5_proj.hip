// t5_proj.hip -- a group of up to 8 bias-free linear maps that share their input rows (the q / k / v, the o and the
// cross-attention K/V projections of modules/t5.py, proj_impl = "hip") as one launch forward and at most two backward
// (gfx950; semantics and arithmetic contract in include/rqhip.h).  The operand layout, the group order, the chain rule,
// the operand loaders and the weight-gradient rule are csrc/t5_matmul.h's, which csrc/t5_ffn.hip uses too.
//
// Row kernel (forward, and the data gradient with the weights in the other orientation).  A workgroup of 4 waves owns
// a tile of 16 rows (more for long batches, below) and ONE chunk of 128 output columns, 32 per wave: grid (row tiles, chunks).  The chain order depends on the
// reduction length alone, so splitting the columns over the grid changes no bit, and it is what fills the device: the
// decoder's 256 rows are 16 row tiles, times 9 chunks for q / k / v at inner = 384.  A chunk's weights are read once
// per row tile whatever the split, so the split costs only the repeated reads of the tile's input rows, which the four
// waves of a workgroup and the workgroups of neighbouring chunks find in L1 / L2.  With one chunk per workgroup there
// is no walk, no resident second accumulator and no barrier, so the rows are not staged in LDS: a lane loads its
// row's 8 terms of a group as two float4 straight from memory (128 contiguous bytes per row and group).
//   forward   the output columns are the n * d_out concatenated columns of y[0] .. y[n - 1]; d_out is a multiple of
//             32, so a wave's 32 columns lie in one y[j].  The reduction runs over d_in.
//   d_x       the output columns are d_x's d_in; the reduction runs over the concatenated (j, term) of the d_y[j] that
//             are not NULL, in ascending j: a chain is 128 consecutive terms of that concatenation.
// Two groups' operands are kept in registers: while the matrix instructions of one run, the next one's loads are in
// flight.
// Row-tile height: 16 rows up to 8192 rows, 32 up to 16384, 64 above.  A workgroup reads its chunk's weights from L2
// whatever the height, so a taller tile divides that traffic; short batches (the model's 5184 and 256 rows at batch 64)
// are short of workgroups instead and keep 16.  The height follows N alone, and the chains do not depend on it.
//
// Weight-gradient kernel: every 32 x 32 tile of every wanted d_w[j] has one owning workgroup, which reduces d_y[j]^T . x
// over all N rows by the weight-gradient rule of csrc/t5_matmul.h.
//
// Second arithmetic, "bf16" (template parameter BF, entry points rqhip_t5_proj_*_bf16), and weight images (template
// parameter IMG of the row kernel, with BF only; entry points rqhip_t5_proj_*_bf16w): as csrc/t5_ffn.hip's.  The images
// (csrc/t5_images.hip) are read along their rows, forward w16[j] [d_out, d_in], d_x the TRANSPOSED images w16t[j]
// [d_in, d_out], and d_x's lanes serve column 16 ct + i like the forward's.  Bits are the BF arm's.
#include <type_traits>

#include "rqhip_common.h"
#include "t5_common.h"
#include "t5_matmul.h"

namespace rqhip {

namespace {

constexpr int kProjMaxD = 512, kProjMaxN = 8;
constexpr int kProjChunk = 128;        // output columns per workgroup of the row kernel: 32 per wave
constexpr long long kProjTallFrom = 16384;   // rows above which a row tile is 64 high (32 above half of it)

bool proj_supported(int d_in, int d_out, int n) {
    return d_in >= 32 && d_in <= kProjMaxD && d_in % 32 == 0 && d_out >= 32 && d_out <= kProjMaxD && d_out % 32 == 0 &&
           n >= 1 && n <= kProjMaxN;
}

struct ProjRows {
    const float *a[kProjMaxN];      // forward: a[0] = x; d_x: the d_y[j] that are not NULL, in ascending j
    long long ld_a[kProjMaxN];
    const float *w[kProjMaxN];      // the weights [d_out, d_in] that go with y[j] (forward) or with a[j] (d_x).  IMG: the
                                    // bf16 images behind these pointers, forward [d_out, d_in], d_x transposed [d_in, d_out]
    float *out[kProjMaxN];          // forward: y[j]; d_x: out[0] = d_x
    long long ld_o[kProjMaxN];
    long long N;
    int n, d_in, d_out;
};

// RT: 16-row tiles per workgroup; BF: the "bf16" arithmetic (the operands are rounded as the fragments are packed); IMG:
// the weights are bf16 images read along their rows (d_x's are the transposed ones)
template <bool BWD, int RT, bool BF, bool IMG = false>
__global__ __launch_bounds__(256) void t5_proj_rows_kernel(const ProjRows p) {
    static_assert(BF || !IMG, "weight images belong to the bf16 arithmetic");
    constexpr bool KN = BWD && !IMG;               // the reduction runs down the columns of the weights as stored
    using WT = std::conditional_t<IMG, __bf16, float>;
    using WB = std::conditional_t<IMG, bf16x8[2], float[2][8]>;      // a group's weight operand for two column tiles
    const int t = threadIdx.x, lane = t & 63, i = lane & 15, kq = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const long long m0 = (long long)blockIdx.x * (16 * RT);
    const int cw = kProjChunk * (int)blockIdx.y + 32 * w;      // this wave's 32 output columns
    const int d_in = p.d_in, d_out = p.d_out;
    if (cw >= (BWD ? d_in : p.n * d_out)) return;
    const int jo = BWD ? 0 : cw / d_out, c0 = BWD ? cw : cw % d_out;      // the output and the wave's first column in it
    const int ng = (BWD ? d_out : d_in) >> 5;                  // groups per segment of the reduction
    const int total = BWD ? p.n * ng : ng;
    long long arow[RT];      // rows past the batch: a valid row is read, nothing is stored
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) arow[rt] = m0 + 16 * rt + i < p.N ? m0 + 16 * rt + i : p.N - 1;

    // the steps of the reduction are loaded in order: the next one is group g of segment seg
    int seg = 0, g = 0;
    auto load = [&](float (&a)[RT][8], WB &b) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
            load_a(p.a[seg] + (size_t)arow[rt] * (size_t)p.ld_a[seg] + 32 * g + 8 * kq, a[rt]);
        if constexpr (IMG) {       // row c0 + i of the image: the ld terms of the output column's reduction
            const size_t ld = BWD ? (size_t)d_out : (size_t)d_in;
            load_b(reinterpret_cast<const WT *>(p.w[BWD ? seg : jo]) + (size_t)(c0 + i) * ld + 32 * g + 8 * kq, ld, b);
        } else {
            const float *at = BWD ? p.w[seg] + (size_t)(32 * g + 8 * kq) * d_in + c0 + 2 * i
                                  : p.w[jo] + (size_t)(c0 + i) * d_in + 32 * g + 8 * kq;
            load_b<BWD>(at, (size_t)d_in, b);
        }
        if (++g == ng) g = 0, ++seg;
    };
    f32x4 sum[RT][2], run[RT][2];      // the sum of the finished chains; the running chain
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) sum[rt][ct] = run[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    float a0[RT][8];
    WB b0;
    float a1[RT][8];
    WB b1;
    load(a0, b0);
    for (int it = 0; it < total; it += 2) {
        if (it + 1 < total) load(a1, b1);
        T5_FENCE; mma<RT, BF>(a0, b0, run); T5_FENCE;
        if (it + 1 < total) {
            if (it + 2 < total) load(a0, b0);
            T5_FENCE; mma<RT, BF>(a1, b1, run); T5_FENCE;
        }
        // kChainGroups is even: a chain ends behind an odd step, or with the reduction
        if (((it + 1) & (kChainGroups - 1)) == kChainGroups - 1 || it + 2 >= total) chain_close<RT>(sum, run);
    }
    static_assert(kChainGroups % 2 == 0, "chains are closed after every second step");

    // sum[rt][ct][r]: row 16 rt + 4 kq + r; column 16 ct + i (forward, images) or 2 i + ct (d_x) of the wave's 32
    float *o = p.out[jo] + c0;
    const size_t ldo = (size_t)p.ld_o[jo];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long grow = m0 + 16 * rt + 4 * kq + r;
            if (grow >= p.N) continue;
            if constexpr (KN) {
                *reinterpret_cast<f32x2 *>(o + (size_t)grow * ldo + 2 * i) = f32x2{sum[rt][0][r], sum[rt][1][r]};
            } else {
                o[(size_t)grow * ldo + i] = sum[rt][0][r];
                o[(size_t)grow * ldo + 16 + i] = sum[rt][1][r];
            }
        }
}

struct ProjWgrad {
    const float *dy[kProjMaxN];     // the jobs: d_w[k] [d_out, d_in] = dy[k]^T . x
    long long ld_dy[kProjMaxN];
    float *dw[kProjMaxN];
    const float *x;
    long long ld_x;
    long long N;
    int d_in, d_out;
    int tiles;                      // 32 x 32 tiles per job: workgroup b owns tile b % tiles of job b / tiles
};

// BF: the "bf16" arithmetic; the lane's eight rows 4 ks + kq of a block are the elements j = ks of both fragments
template <bool BF>
__global__ __launch_bounds__(256) void t5_proj_wgrad_kernel(const ProjWgrad p) {
    __shared__ float red[4 * 32 * 33];
    const int t = threadIdx.x, lane = t & 63, i = lane & 15, kq = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int job = (int)blockIdx.x / p.tiles, tile = (int)blockIdx.x % p.tiles;
    // out [rows of P's columns, columns of Q's columns] = sum_n P[n][a0 + .] Q[n][b0 + .]
    const float *P = p.dy[job], *Q = p.x;
    const size_t lp = (size_t)p.ld_dy[job], lq = (size_t)p.ld_x;
    float *out = p.dw[job];
    const int a0 = 32 * (tile / (p.d_in >> 5)), b0 = 32 * (tile % (p.d_in >> 5));

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
        out[(size_t)(a0 + row) * p.d_in + b0 + col] = v;
    }
}

// The checks the entry points share; `who` names the entry point in the message.
int proj_check(const char *who, int n, int64_t N, int d_in, int d_out) {
    if (N < 0 || d_in < 1 || d_out < 1 || n < 0) {
        set_error("%s: bad sizes (N=%lld, d_in=%d, d_out=%d, n=%d)", who, (long long)N, d_in, d_out, n);
        return RQHIP_EARG;
    }
    if (!proj_supported(d_in, d_out, n)) {
        set_error("%s: d_in=%d, d_out=%d, n=%d: only multiples of 32 with 32 <= d_in, d_out <= %d and 1 <= n <= %d are "
                  "implemented", who, d_in, d_out, n, kProjMaxD, kProjMaxN);
        return RQHIP_EUNSUPPORTED;
    }
    if (N / 16 >= (1ll << 31) - 1) {
        set_error("%s: N=%lld exceeds 16 rows per workgroup of a 2^31 grid", who, (long long)N);
        return RQHIP_EUNSUPPORTED;
    }
    return RQHIP_OK;
}

// a row stride the float4 loads can take: at least the row, a multiple of 4
bool proj_ld_ok(int64_t ld, int width) { return ld >= width && ld % 4 == 0; }

// 16-row tiles per workgroup: a function of N alone, and the chains do not depend on it
int proj_row_tiles(long long N) { return N > kProjTallFrom ? 4 : N > kProjTallFrom / 2 ? 2 : 1; }

template <bool BWD, int RT, bool BF, bool IMG>
int proj_rows_launch_rt(const ProjRows &a, int cols, hipStream_t s) {
    const dim3 grid((unsigned)((a.N + 16 * RT - 1) / (16 * RT)), (unsigned)((cols + kProjChunk - 1) / kProjChunk));
    hipLaunchKernelGGL((t5_proj_rows_kernel<BWD, RT, BF, IMG>), grid, dim3(256), 0, s, a);
    RQ_CHECK_LAUNCH("t5_proj_rows_kernel");
    return RQHIP_OK;
}

template <bool BWD, bool BF, bool IMG>
int proj_rows_launch(const ProjRows &a, int cols, hipStream_t s) {
    const int rt = proj_row_tiles(a.N);
    if (rt == 1) return proj_rows_launch_rt<BWD, 1, BF, IMG>(a, cols, s);
    if (rt == 2) return proj_rows_launch_rt<BWD, 2, BF, IMG>(a, cols, s);
    return proj_rows_launch_rt<BWD, 4, BF, IMG>(a, cols, s);
}

// the entry points of both arithmetics; `who` names the one called in the messages.  IMG: w[j] are the bf16 images the
// call reads (forward w16[j], backward the transposed w16t[j])
template <bool BF, bool IMG = false>
int proj_fwd(const char *who, const float *x, int64_t ld_x, const float *const *w, float *const *y, const int64_t *ld_y,
             int n, int64_t N, int d_in, int d_out, rqhip_stream_t stream) {
    const int rc = proj_check(who, n, N, d_in, d_out);
    if (rc != RQHIP_OK) return rc;
    if (N == 0) return RQHIP_OK;
    if (any_null(x, w, y, ld_y)) {
        set_error("%s: null pointer (x, w, y, ld_y)", who);
        return RQHIP_EARG;
    }
    ProjRows a = {};
    a.a[0] = x, a.ld_a[0] = ld_x, a.N = N, a.n = n, a.d_in = d_in, a.d_out = d_out;
    for (int j = 0; j < n; ++j) {
        if (!w[j] || !y[j]) {
            set_error("%s: null pointer (w[%d] or y[%d])", who, j, j);
            return RQHIP_EARG;
        }
        if (ld_y[j] < d_out) {
            set_error("%s: ld_y[%d]=%lld is less than d_out=%d", who, j, (long long)ld_y[j], d_out);
            return RQHIP_EARG;
        }
        if (!aligned16(w[j]) || (reinterpret_cast<uintptr_t>(y[j]) & 3)) {
            set_error("%s: w[%d] must be 16-byte aligned and y[%d] 4-byte aligned", who, j, j);
            return RQHIP_EARG;
        }
        a.w[j] = w[j], a.out[j] = y[j], a.ld_o[j] = ld_y[j];
    }
    if (!proj_ld_ok(ld_x, d_in) || !aligned16(x)) {
        set_error("%s: x must be 16-byte aligned with a row stride ld_x=%lld >= d_in=%d that is a multiple of 4", who,
                  (long long)ld_x, d_in);
        return RQHIP_EARG;
    }
    return proj_rows_launch<false, BF, IMG>(a, n * d_out, reinterpret_cast<hipStream_t>(stream));
}

template <bool BF, bool IMG = false>
int proj_bwd(const char *who, const float *x, int64_t ld_x, const float *const *w, const float *const *d_y,
             const int64_t *ld_dy, int n, int64_t N, int d_in, int d_out, float *d_x, float *const *d_w,
             rqhip_stream_t stream) {
    const int rc = proj_check(who, n, N, d_in, d_out);
    if (rc != RQHIP_OK) return rc;
    if (N == 0) return RQHIP_OK;
    if (any_null(x, w, d_y, ld_dy)) {
        set_error("%s: null pointer (x, w, d_y, ld_dy)", who);
        return RQHIP_EARG;
    }
    if (!proj_ld_ok(ld_x, d_in) || !aligned16(x) || !aligned16(d_x)) {
        set_error("%s: x and d_x must be 16-byte aligned, x with a row stride ld_x=%lld >= d_in=%d that is a multiple of 4",
                  who, (long long)ld_x, d_in);
        return RQHIP_EARG;
    }
    ProjRows a = {};       // the data gradient over the d_y[j] that are there
    ProjWgrad q = {};      // the weight gradients that are wanted and have a d_y[j]
    int na = 0, nq = 0;
    for (int j = 0; j < n; ++j) {
        if (!w[j]) {
            set_error("%s: null pointer (w[%d])", who, j);
            return RQHIP_EARG;
        }
        if (!d_y[j]) continue;
        if (!proj_ld_ok(ld_dy[j], d_out) || !aligned16(d_y[j]) || !aligned16(w[j])) {
            set_error("%s: d_y[%d] and w[%d] must be 16-byte aligned, d_y[%d] with a row stride ld_dy[%d]=%lld >= d_out=%d "
                      "that is a multiple of 4", who, j, j, j, j, (long long)ld_dy[j], d_out);
            return RQHIP_EARG;
        }
        a.a[na] = d_y[j], a.ld_a[na] = ld_dy[j], a.w[na] = w[j], ++na;
        if (d_w && d_w[j]) {
            if (reinterpret_cast<uintptr_t>(d_w[j]) & 3) {
                set_error("%s: d_w[%d] must be 4-byte aligned", who, j);
                return RQHIP_EARG;
            }
            q.dy[nq] = d_y[j], q.ld_dy[nq] = ld_dy[j], q.dw[nq] = d_w[j], ++nq;
        }
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (d_x && na) {
        a.out[0] = d_x, a.ld_o[0] = d_in, a.N = N, a.n = na, a.d_in = d_in, a.d_out = d_out;
        const int rc1 = proj_rows_launch<true, BF, IMG>(a, d_in, s);
        if (rc1 != RQHIP_OK) return rc1;
    }
    if (nq) {
        q.x = x, q.ld_x = ld_x, q.N = N, q.d_in = d_in, q.d_out = d_out;
        q.tiles = (d_in / 32) * (d_out / 32);
        hipLaunchKernelGGL(t5_proj_wgrad_kernel<BF>, dim3((unsigned)(nq * q.tiles)), dim3(256), 0, s, q);
        RQ_CHECK_LAUNCH("t5_proj_wgrad_kernel");
    }
    return RQHIP_OK;
}

}  // namespace

}  // namespace rqhip

using namespace rqhip;

extern "C" int rqhip_t5_proj_supported(int d_in, int d_out, int n) { return proj_supported(d_in, d_out, n) ? 1 : 0; }

extern "C" int rqhip_t5_proj_fwd(const float *x, int64_t ld_x, const float *const *w, float *const *y, const int64_t *ld_y,
                                 int n, int64_t N, int d_in, int d_out, rqhip_stream_t stream) {
    return proj_fwd<false>("t5_proj_fwd", x, ld_x, w, y, ld_y, n, N, d_in, d_out, stream);
}

extern "C" int rqhip_t5_proj_fwd_bf16(const float *x, int64_t ld_x, const float *const *w, float *const *y,
                                      const int64_t *ld_y, int n, int64_t N, int d_in, int d_out, rqhip_stream_t stream) {
    return proj_fwd<true>("t5_proj_fwd_bf16", x, ld_x, w, y, ld_y, n, N, d_in, d_out, stream);
}

extern "C" int rqhip_t5_proj_bwd(const float *x, int64_t ld_x, const float *const *w, const float *const *d_y,
                                 const int64_t *ld_dy, int n, int64_t N, int d_in, int d_out, float *d_x,
                                 float *const *d_w, rqhip_stream_t stream) {
    return proj_bwd<false>("t5_proj_bwd", x, ld_x, w, d_y, ld_dy, n, N, d_in, d_out, d_x, d_w, stream);
}

extern "C" int rqhip_t5_proj_bwd_bf16(const float *x, int64_t ld_x, const float *const *w, const float *const *d_y,
                                      const int64_t *ld_dy, int n, int64_t N, int d_in, int d_out, float *d_x,
                                      float *const *d_w, rqhip_stream_t stream) {
    return proj_bwd<true>("t5_proj_bwd_bf16", x, ld_x, w, d_y, ld_dy, n, N, d_in, d_out, d_x, d_w, stream);
}

extern "C" int rqhip_t5_proj_fwd_bf16w(const float *x, int64_t ld_x, const rqhip_bf16_t *const *w16, float *const *y,
                                       const int64_t *ld_y, int n, int64_t N, int d_in, int d_out, rqhip_stream_t stream) {
    return proj_fwd<true, true>("t5_proj_fwd_bf16w", x, ld_x, reinterpret_cast<const float *const *>(w16), y, ld_y, n, N, d_in,
                                d_out, stream);
}

extern "C" int rqhip_t5_proj_bwd_bf16w(const float *x, int64_t ld_x, const rqhip_bf16_t *const *w16t, const float *const *d_y,
                                       const int64_t *ld_dy, int n, int64_t N, int d_in, int d_out, float *d_x,
                                       float *const *d_w, rqhip_stream_t stream) {
    return proj_bwd<true, true>("t5_proj_bwd_bf16w", x, ld_x, reinterpret_cast<const float *const *>(w16t), d_y, ld_dy, n, N,
                                d_in, d_out, d_x, d_w, stream);
}

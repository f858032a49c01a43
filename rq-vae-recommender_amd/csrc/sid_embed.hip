// sid_embed.hip -- the retrieval model's input embedding as one launch forward and one backward (gfx950): the index
// computation and row gather that turn semantic ids into a T5 stack's inputs_embeds, and the segmented row sum that is
// its gradient (modules/model.py, embed_impl = "hip"; semantics in include/rqhip.h).
//
// One "row plan" serves the encoder and the decoder front.  An output row b has T = has_prefix + items * (L + has_sep)
// positions: an optional prefix (a user-table row, or a [1, d] parameter for every b), then per item its L id positions
// and an optional separator.
//
// Forward: one wave64 per output position; lane l copies the float4s l, l + 64, l + 128, l + 192 of its source row.
//
// Backward: one workgroup of four waves per DESTINATION row -- the V = L * K table rows, then the separator, then the
// prefix rows.  It scans its domain (the B * items * L id tokens for a table row, the B * items items for the separator,
// the B rows for a prefix row) in chunks of 1024 tokens.  A chunk's matches are compacted in ascending token order into
// an LDS list: a ballot and a popcount give each match its rank inside its wave, the waves' counts are added in wave
// order.  The list holds one chunk, so its capacity never depends on the data.  With G = max(1, 256 / (d / 4)) threads per
// float4 column, thread (g, c) adds entries g, g + G, g + 2G, ... of the list in that order from +0, the G sums of a
// column are added in ascending g, and the chunks' sums are added in ascending order from +0: no chain is longer than
// 1024 / G + G + chunks, there are no atomics, and the order is a function of the shape and the ids alone.
#include "rqhip_common.h"
#include "t5_common.h"

namespace rqhip {

namespace {

constexpr int kSeMaxD = 1024;
constexpr int kSeMaxL = 8;
constexpr int kSeWaves = 4;
constexpr int kSeThreads = kSeWaves * RQ_WAVE;
constexpr int kSeRounds = 4;                                // tokens per thread and chunk
constexpr int kSeWaveChunk = kSeRounds * RQ_WAVE;           // consecutive tokens one wave scans per chunk
constexpr int kSeChunk = kSeWaves * kSeWaveChunk;           // 1024

bool se_supported(int d, int L) { return d >= 4 && d <= kSeMaxD && d % 4 == 0 && L >= 1 && L <= kSeMaxL; }

struct SePlan {
    const long long *ids;         // [B, items * ld_item]
    const void *mask;             // the same layout, bool (mask_elt 1) or int64 (8); nullptr = all ones
    const long long *prefix_idx;  // row b at b * prefix_idx_ld; nullptr = prefix row 0 for every b
    long long prefix_idx_ld, prefix_rows, B;
    int mask_elt, items, L, ld_item, K, d, has_sep, has_prefix;
};

__device__ __forceinline__ int se_positions(const SePlan &p) { return p.has_prefix + p.items * (p.L + p.has_sep); }

__device__ __forceinline__ long long se_mask(const SePlan &p, size_t e) {
    if (!p.mask) return 1;
    if (p.mask_elt == 1) return reinterpret_cast<const unsigned char *>(p.mask)[e] != 0;
    return reinterpret_cast<const long long *>(p.mask)[e] != 0;
}

// element of ids / mask that holds level h of item i of row b
__device__ __forceinline__ size_t se_element(const SePlan &p, long long b, int i, int h) {
    return ((size_t)b * (size_t)p.items + (size_t)i) * (size_t)p.ld_item + (size_t)h;
}

// torch.remainder: the result has the sign of the (positive) divisor
__device__ __forceinline__ long long se_prefix_row(const SePlan &p, long long b) {
    if (!p.prefix_idx) return 0;
    const long long r = p.prefix_idx[b * p.prefix_idx_ld] % p.prefix_rows;
    return r < 0 ? r + p.prefix_rows : r;
}

__global__ __launch_bounds__(kSeThreads) void sid_embed_fwd_kernel(SePlan p, const float *table, const float *sep,
                                                                   const float *prefix_table, float *x,
                                                                   unsigned char *mask_out) {
    const int lane = threadIdx.x & (RQ_WAVE - 1), wave = threadIdx.x / RQ_WAVE;
    const int T = se_positions(p);
    const long long row = (long long)blockIdx.x * kSeWaves + wave;   // b * T + t, below 2^31 (se_check)
    if (row >= p.B * T) return;
    const int b = (int)row / T, t = (int)row % T;
    const float *src;
    long long m = 1;
    if (p.has_prefix && t == 0) {
        src = prefix_table + (size_t)se_prefix_row(p, b) * (size_t)p.d;
    } else {
        const int per_item = p.L + p.has_sep, u = t - p.has_prefix;
        const int i = u / per_item, h = u % per_item;
        const size_t e = se_element(p, b, i, h == p.L ? p.L - 1 : h);   // a separator copies its item's last level
        m = se_mask(p, e);
        if (h == p.L) {
            src = sep;
        } else {
            const long long V = (long long)p.L * p.K;
            long long idx = (p.ids[e] + (long long)h * p.K) * m;
            idx = idx < 0 ? 0 : (idx >= V ? V - 1 : idx);                // a bad id reads a valid row, never faults
            src = table + (size_t)idx * (size_t)p.d;
        }
    }
    float *dst = x + (size_t)row * (size_t)p.d;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = 4 * (lane + RQ_WAVE * k);
        if (c < p.d) *reinterpret_cast<f32x4 *>(dst + c) = *reinterpret_cast<const f32x4 *>(src + c);
    }
    if (mask_out && lane == 0) mask_out[row] = (unsigned char)m;
}

enum { kSeTable = 0, kSeSep = 1, kSePrefix = 2 };

// the position b * T + t of d_x that token n of a destination's domain adds to destination row r, or -1 (every domain
// is at most B * T tokens, below 2^31: se_check)
__device__ __forceinline__ int se_match(const SePlan &p, int kind, long long r, int n, int T) {
    if (kind == kSeTable) {
        const int per_row = p.items * p.L;
        const int b = n / per_row, u = n % per_row, i = u / p.L, h = u % p.L;
        const size_t e = se_element(p, b, i, h);
        const long long idx = (p.ids[e] + (long long)h * p.K) * se_mask(p, e);   // outside [0, V): equals no r, dropped
        return idx == r ? b * T + p.has_prefix + i * (p.L + p.has_sep) + h : -1;
    }
    if (kind == kSeSep) {
        const int b = n / p.items, i = n % p.items;
        return b * T + p.has_prefix + i * (p.L + 1) + p.L;
    }
    return se_prefix_row(p, n) == r ? n * T : -1;
}

// s += the rows list[j], list[j + G], ... of one float4 column, U at a time while U are left: the U loads are
// independent and in flight together, the adds keep the list's order
template <int U>
__device__ __forceinline__ void se_add_run(f32x4 &s, const float *col, const int *list, int &j, int G, int count, int d) {
    for (; j + (U - 1) * G < count; j += U * G) {
        f32x4 a[U];
#pragma unroll
        for (int u = 0; u < U; ++u) a[u] = *reinterpret_cast<const f32x4 *>(col + (size_t)list[j + u * G] * (size_t)d);
#pragma unroll
        for (int u = 0; u < U; ++u) s = s + a[u];
    }
}

__global__ __launch_bounds__(kSeThreads) void sid_embed_bwd_kernel(SePlan p, const float *d_x, float *d_table,
                                                                   float *d_sep, float *d_prefix) {
    __shared__ int list[kSeChunk];
    __shared__ int wave_count[kSeWaves];
    __shared__ f32x4 part[kSeThreads];
    const int lane = threadIdx.x & (RQ_WAVE - 1), wave = threadIdx.x / RQ_WAVE;
    const int T = se_positions(p);
    const long long V = (long long)p.L * p.K;

    // this workgroup's destination row and the domain it scans (all of it workgroup-uniform)
    long long r = blockIdx.x, domain;
    int kind;
    float *dst;
    if (r < V) {
        kind = kSeTable, domain = p.B * p.items * p.L;
        dst = d_table ? d_table + (size_t)r * (size_t)p.d : nullptr;
    } else if (p.has_sep && r == V) {
        kind = kSeSep, domain = p.B * p.items;
        dst = d_sep;
    } else {
        r -= V + p.has_sep;
        kind = kSePrefix, domain = p.B;
        dst = d_prefix ? d_prefix + (size_t)r * (size_t)p.d : nullptr;
    }
    if (!dst) return;   // that gradient is not wanted

    const int cols = p.d / 4;                       // float4 columns
    const int G = cols < kSeThreads ? kSeThreads / cols : 1;
    const int g = threadIdx.x / cols, c = threadIdx.x % cols;
    const bool active = g < G;
    const float *col = d_x + 4 * c;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};

    for (long long chunk0 = 0; chunk0 < domain; chunk0 += kSeChunk) {
        // each wave takes kSeWaveChunk consecutive tokens, 64 at a time: ranks ascend with the token
        int pos[kSeRounds], rank[kSeRounds], mine = 0;
#pragma unroll
        for (int rd = 0; rd < kSeRounds; ++rd) {
            const long long n = chunk0 + wave * kSeWaveChunk + rd * RQ_WAVE + lane;
            pos[rd] = n < domain ? se_match(p, kind, r, (int)n, T) : -1;
            const unsigned long long hit = __ballot(pos[rd] >= 0);
            rank[rd] = mine + __popcll(hit & ((1ull << lane) - 1ull));
            mine += __popcll(hit);
        }
        if (lane == 0) wave_count[wave] = mine;
        __syncthreads();
        int base = 0, count = 0;
#pragma unroll
        for (int w = 0; w < kSeWaves; ++w) {
            if (w < wave) base += wave_count[w];
            count += wave_count[w];
        }
#pragma unroll
        for (int rd = 0; rd < kSeRounds; ++rd)
            if (pos[rd] >= 0) list[base + rank[rd]] = pos[rd];   // base + rank < count <= kSeChunk
        __syncthreads();
        if (count == 0) continue;                  // workgroup-uniform

        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        if (active) {   // 16 loads in flight, then 4, then 1; always added in list order
            int j = g;
            se_add_run<16>(s, col, list, j, G, count, p.d);
            se_add_run<4>(s, col, list, j, G, count, p.d);
            se_add_run<1>(s, col, list, j, G, count, p.d);
        }
        if (G > 1) {                               // the G sums of a column in ascending g
            part[threadIdx.x] = s;
            __syncthreads();
            if (g == 0) {
                s = part[c];
                for (int k = 1; k < G; ++k) s = s + part[k * cols + c];
            }
        }
        if (g == 0) acc = acc + s;
        // no barrier here: the next chunk writes wave_count before, list and part after a barrier every thread reaches
        // only when it has left this chunk
    }
    if (g == 0) *reinterpret_cast<f32x4 *>(dst + 4 * c) = acc;
}

// The checks both entry points share; `who` names the entry point in the message.
int se_check(const char *who, int64_t B, int items, int L, int ld_item, int K, int d, const void *mask, int mask_elt,
             int has_sep, int has_prefix, int64_t prefix_rows) {
    if (B < 0 || items < 1 || K < 1) {
        set_error("%s: bad sizes (B=%lld, items=%d, K=%d)", who, (long long)B, items, K);
        return RQHIP_EARG;
    }
    if (!se_supported(d, L)) {
        set_error("%s: d=%d, L=%d: only d a multiple of 4 in 4 .. %d and L in 1 .. %d are implemented", who, d, L, kSeMaxD,
                  kSeMaxL);
        return RQHIP_EARG;
    }
    if (ld_item < L) {
        set_error("%s: ld_item=%d, need ld_item >= L=%d", who, ld_item, L);
        return RQHIP_EARG;
    }
    if (mask && mask_elt != 1 && mask_elt != 8) {
        set_error("%s: mask element size %d, the mask is bool (1) or int64 (8)", who, mask_elt);
        return RQHIP_EARG;
    }
    if (has_prefix && prefix_rows < 1) {
        set_error("%s: prefix_rows=%lld with a prefix table", who, (long long)prefix_rows);
        return RQHIP_EARG;
    }
    const long long T = (has_prefix ? 1 : 0) + (long long)items * (L + (has_sep ? 1 : 0));
    const long long grid = (long long)L * K + (has_prefix ? prefix_rows : 0) + 1;
    if (T >= (1ll << 31) || B * T >= (1ll << 31) || (long long)items * ld_item >= (1ll << 31) || grid >= (1ll << 31)) {
        set_error("%s: B=%lld rows of T=%lld positions, or L*K + prefix_rows = %lld destination rows, exceed 2^31", who,
                  (long long)B, T, grid);
        return RQHIP_EUNSUPPORTED;
    }
    return RQHIP_OK;
}

}  // namespace

}  // namespace rqhip

using namespace rqhip;

extern "C" int rqhip_sid_embed_supported(int d, int L) { return se_supported(d, L); }

extern "C" size_t rqhip_sid_embed_bwd_workspace_bytes(int64_t B, int items, int L, int K, int d) {
    (void)B, (void)items, (void)L, (void)K, (void)d;
    return 0;   // one workgroup per destination row keeps every partial sum in LDS: nothing is staged in global memory
}

extern "C" int rqhip_sid_embed_fwd(const int64_t *ids, const void *mask, int mask_elt_size, int64_t B, int items, int L,
                                   int ld_item, int K, int d, const float *table, const float *sep,
                                   const float *prefix_table, const int64_t *prefix_idx, int64_t prefix_idx_ld,
                                   int64_t prefix_rows, float *x, uint8_t *mask_out, rqhip_stream_t stream) {
    const int rc = se_check("sid_embed_fwd", B, items, L, ld_item, K, d, mask, mask_elt_size, sep != nullptr,
                            prefix_table != nullptr, prefix_rows);
    if (rc != RQHIP_OK) return rc;
    if (B == 0) return RQHIP_OK;
    if (any_null(ids, table, x)) {
        set_error("sid_embed_fwd: null pointer (ids, table, x)");
        return RQHIP_EARG;
    }
    if (!all_aligned16(table, sep, prefix_table, x)) {
        set_error("sid_embed_fwd: table, sep, prefix_table and x must be 16-byte aligned");
        return RQHIP_EARG;
    }
    SePlan p;
    p.ids = reinterpret_cast<const long long *>(ids), p.mask = mask;
    p.prefix_idx = prefix_table ? reinterpret_cast<const long long *>(prefix_idx) : nullptr;
    p.prefix_idx_ld = prefix_idx_ld, p.prefix_rows = prefix_rows, p.B = B;
    p.mask_elt = mask_elt_size, p.items = items, p.L = L, p.ld_item = ld_item, p.K = K, p.d = d;
    p.has_sep = sep != nullptr, p.has_prefix = prefix_table != nullptr;
    const long long rows = B * (p.has_prefix + (long long)items * (L + p.has_sep));
    hipLaunchKernelGGL(sid_embed_fwd_kernel, dim3((unsigned)((rows + kSeWaves - 1) / kSeWaves)), dim3(kSeThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), p, table, sep, prefix_table, x, mask_out);
    RQ_CHECK_LAUNCH("sid_embed_fwd_kernel");
    return RQHIP_OK;
}

extern "C" int rqhip_sid_embed_bwd(const float *d_x, const int64_t *ids, const void *mask, int mask_elt_size, int64_t B,
                                   int items, int L, int ld_item, int K, int d, int has_sep, int has_prefix,
                                   const int64_t *prefix_idx, int64_t prefix_idx_ld, int64_t prefix_rows, float *d_table,
                                   float *d_sep, float *d_prefix, void *workspace, size_t workspace_bytes,
                                   rqhip_stream_t stream) {
    const int rc = se_check("sid_embed_bwd", B, items, L, ld_item, K, d, mask, mask_elt_size, has_sep, has_prefix,
                            prefix_rows);
    if (rc != RQHIP_OK) return rc;
    if (B == 0) return RQHIP_OK;
    if (any_null(d_x, ids)) {
        set_error("sid_embed_bwd: null pointer (d_x, ids)");
        return RQHIP_EARG;
    }
    if ((d_sep && !has_sep) || (d_prefix && !has_prefix)) {
        set_error("sid_embed_bwd: d_sep without has_sep, or d_prefix without has_prefix");
        return RQHIP_EARG;
    }
    if (!all_aligned16(d_x, d_table, d_sep, d_prefix)) {
        set_error("sid_embed_bwd: d_x, d_table, d_sep and d_prefix must be 16-byte aligned");
        return RQHIP_EARG;
    }
    if (workspace_bytes < rqhip_sid_embed_bwd_workspace_bytes(B, items, L, K, d)) {
        set_error("sid_embed_bwd: workspace of %zu bytes, rqhip_sid_embed_bwd_workspace_bytes = %zu", workspace_bytes,
                  rqhip_sid_embed_bwd_workspace_bytes(B, items, L, K, d));
        return RQHIP_EARG;
    }
    (void)workspace;
    if (!d_table && !d_sep && !d_prefix) return RQHIP_OK;
    SePlan p;
    p.ids = reinterpret_cast<const long long *>(ids), p.mask = mask;
    p.prefix_idx = has_prefix ? reinterpret_cast<const long long *>(prefix_idx) : nullptr;
    p.prefix_idx_ld = prefix_idx_ld, p.prefix_rows = prefix_rows, p.B = B;
    p.mask_elt = mask_elt_size, p.items = items, p.L = L, p.ld_item = ld_item, p.K = K, p.d = d;
    p.has_sep = has_sep ? 1 : 0, p.has_prefix = has_prefix ? 1 : 0;
    const long long grid = (long long)L * K + p.has_sep + (p.has_prefix ? prefix_rows : 0);
    hipLaunchKernelGGL(sid_embed_bwd_kernel, dim3((unsigned)grid), dim3(kSeThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), p, d_x, d_table, d_sep, d_prefix);
    RQ_CHECK_LAUNCH("sid_embed_bwd_kernel");
    return RQHIP_OK;
}

// beam_step.hip -- one hierarchy step of EncoderDecoderRetrievalModel.generate as one launch (gfx950).
//
// Reference (modules/model.py, generate): per step a softmax over K codes for every row, torch.multinomial without
// replacement, a gather and a log, the [N, P, h] prefix-equality tensor of _check_valid_prefix, a masked_fill, a full
// sort of beams_in * n_cands scores per user and four gathers and a cat -- about fifteen launches and the host read of
// multinomial's input check.  Here one workgroup owns one user and its beams_in rows:
//
//   phase A (one wave per row, rows strided over the waves): p = softmax(logits[r]) in fp32; key[c] = p[c] / noise[r, c]
//            (ATen's multinomial without replacement: topk(p / q, n), q ~ Exp(1)); the n largest keys, ties to the lower
//            code, by a tournament: every lane keeps the best of the codes c == lane (mod 64), the wave takes the maximum,
//            the winning lane retires its code and rescans its own slots.  Each lane only touches its own LDS slots.
//            Candidate j = beam * n + s gets score = log(p[sample]) (+ the parent beam's score when h > 0).
//   phase B (all threads): a candidate whose (h+1)-prefix is not in the corpus scores -inf -- the same exact hash
//            probe as rqhip_prefix_lookup (csrc/sid_hash.h), confirmed against the corpus row.
//   phase C (wave 0): the k best candidates, ties (-inf included) to the lower j, by the same tournament.
//   phase D (all threads): ids = parent ids ++ sample, scores, the global parent row.
//
// Keys are 64-bit: the order-preserving image of the fp32 value in the high word, ~index in the low word, so every key
// is distinct and the maximum is unique; 0 is below every real key and marks a retired slot.  No atomics, fixed
// reduction orders: the same bits on every run.  No allocation, copy or sync in the launch path (graph-capturable once
// the LDS attribute has been raised by a first eager call, as everywhere in this library).
//
// The exact step of model.beam_impl = "exact" (rqhip_beam_topk_step, no noise: every code is a candidate) shares the keys
// and the tournament; it is described at beam_topk_step_kernel below.
#include "rqhip_common.h"
#include "sid_hash.h"

namespace rqhip {

namespace {

constexpr int kBeamMaxK = 4096;      // codes per hierarchy
constexpr int kBeamMaxCands = 64;    // samples per row
constexpr int kBeamMaxTopK = 64;     // beams kept per user
constexpr int kBeamMaxWaves = 4;

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int off = 1; off < RQ_WAVE; off <<= 1) {
        const unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
        const unsigned olo = (unsigned)__shfl_xor((int)lo, off, RQ_WAVE);
        const unsigned ohi = (unsigned)__shfl_xor((int)hi, off, RQ_WAVE);
        const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
    for (int off = 1; off < RQ_WAVE; off <<= 1) v = fmaxf(v, __shfl_xor(v, off, RQ_WAVE));
    return v;
}

// xor butterfly: both partners add the same two values, so every lane ends with the same bits
__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int off = 1; off < RQ_WAVE; off <<= 1) v = v + __shfl_xor(v, off, RQ_WAVE);
    return v;
}

// total order of fp32 as unsigned: -inf -> 0x007fffff ... +0 -> 0x80000000 ... +inf
__device__ __forceinline__ unsigned f32_order(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float f32_from_order(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

__device__ __forceinline__ unsigned long long tour_key(unsigned v, unsigned idx) {
    return v ? (((unsigned long long)v << 32) | (0xffffffffu - idx)) : 0ull;
}

// best key among the slots idx = lane + 64 t < count of `vals`
__device__ __forceinline__ unsigned long long lane_best(const unsigned *vals, int count, int lane) {
    unsigned long long best = 0;
    for (int idx = lane; idx < count; idx += RQ_WAVE) {
        const unsigned long long key = tour_key(vals[idx], (unsigned)idx);
        best = key > best ? key : best;
    }
    return best;
}

// The `m` largest keys of vals[0, count) in descending order (m <= count).  Calls emit(rank, idx, value) on lane
// rank % 64 for each.  vals must hold no 0 (the retired mark); every slot is read and written by its own lane only.
template <typename Emit>
__device__ __forceinline__ void wave_top(unsigned *vals, int count, int m, int lane, Emit emit) {
    unsigned long long best = lane_best(vals, count, lane);
    for (int r = 0; r < m; ++r) {
        const unsigned long long w = wave_max_u64(best);
        const unsigned idx = 0xffffffffu - (unsigned)w;
        if ((int)(idx & (RQ_WAVE - 1)) == lane) {
            vals[idx] = 0u;
            best = lane_best(vals, count, lane);
        }
        if ((r & (RQ_WAVE - 1)) == lane) emit(r, (int)idx, (unsigned)(w >> 32));
    }
}

__global__ __launch_bounds__(256) void beam_step_kernel(
    const float *__restrict__ logits, long long ld_logits, const float *__restrict__ noise,
    const float *__restrict__ parent_scores, const int64_t *__restrict__ parent_ids, int h, int beams_in, int K,
    int n, int k, const int *__restrict__ table, unsigned mask, const int64_t *__restrict__ corpus, long long N,
    long long ld, int64_t *__restrict__ out_ids, float *__restrict__ out_scores, int64_t *__restrict__ out_parent) {
    extern __shared__ unsigned lds[];
    __shared__ int win_idx[kBeamMaxTopK];
    __shared__ unsigned win_key[kBeamMaxTopK];

    const int nw = blockDim.x / RQ_WAVE;
    const int wave = threadIdx.x / RQ_WAVE, lane = threadIdx.x & (RQ_WAVE - 1);
    const long long b = blockIdx.x;
    const int C = beams_in * n;
    unsigned *rowkeys = lds + (size_t)wave * K;  // [K] per wave
    unsigned *ckey = lds + (size_t)nw * K;       // [C] order image of each candidate's score
    int *csamp = reinterpret_cast<int *>(ckey + C);  // [C] sampled code of each candidate

    // ---- phase A: softmax, exponential race, top-n samples per row
    for (int beam = wave; beam < beams_in; beam += nw) {
        const long long row = b * beams_in + beam;
        const float *x = logits + (size_t)row * (size_t)ld_logits;
        const float *q = noise + (size_t)row * (size_t)K;
        float m = -INFINITY;
        for (int c = lane; c < K; c += RQ_WAVE) m = fmaxf(m, x[c]);
        m = wave_max_f32(m);
        float s = 0.f;
        for (int c = lane; c < K; c += RQ_WAVE) s += expf(x[c] - m);
        s = wave_sum_f32(s);
        for (int c = lane; c < K; c += RQ_WAVE) {
            const float p = expf(x[c] - m) / s;
            rowkeys[c] = __float_as_uint(p / q[c]) + 1u;  // keys are >= +0: their bits order them; 0 stays free
        }
        const float base = parent_scores ? parent_scores[row] : 0.f;
        const bool add_base = parent_scores != nullptr;
        wave_top(rowkeys, K, n, lane, [&](int r, int c, unsigned) {
            const float lp = logf(expf(x[c] - m) / s);
            const int j = beam * n + r;
            ckey[j] = f32_order(add_base ? lp + base : lp);
            csamp[j] = c;
        });
    }
    __syncthreads();

    // ---- phase B: -inf unless the (h+1)-prefix occurs in the corpus
    const unsigned neg_inf = f32_order(-INFINITY);
    const size_t slots = (size_t)mask + 1;
    const int *tab = table + (size_t)h * slots;
    for (int j = threadIdx.x; j < C; j += blockDim.x) {
        if (ckey[j] == neg_inf) continue;
        bool found = false;
        if (N > 0) {
            const int beam = j / n;
            const int64_t *par = parent_ids + ((size_t)b * beams_in + beam) * (size_t)h;
            const int64_t samp = csamp[j];
            unsigned hsh = kSidHashSeed;
            for (int t = 0; t < h; ++t) hsh = sid_hash_step(hsh, par[t]);
            hsh = sid_hash_step(hsh, samp);
            unsigned slot = sid_hash_final(hsh) & mask;
            for (;;) {
                const int prev = tab[slot];
                if (prev == -1) break;
                const int64_t *other = corpus + (size_t)prev * (size_t)ld;
                bool same = other[h] == samp;
                for (int t = 0; t < h && same; ++t) same = other[t] == par[t];
                if (same) {
                    found = true;
                    break;
                }
                slot = (slot + 1) & mask;
            }
        }
        if (!found) ckey[j] = neg_inf;
    }
    __syncthreads();

    // ---- phase C: the k best candidates of the user
    if (wave == 0) {
        wave_top(ckey, C, k, lane, [&](int r, int j, unsigned v) {
            win_idx[r] = j;
            win_key[r] = v;
        });
    }
    __syncthreads();

    // ---- phase D: outputs
    const int h1 = h + 1;
    for (int e = threadIdx.x; e < k * h1; e += blockDim.x) {
        const int i = e / h1, t = e - i * h1;
        const int j = win_idx[i];
        const int beam = j / n;
        const int64_t v = t < h ? parent_ids[((size_t)b * beams_in + beam) * (size_t)h + t] : (int64_t)csamp[j];
        out_ids[((size_t)b * k + i) * (size_t)h1 + t] = v;
    }
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        out_scores[(size_t)b * k + i] = f32_from_order(win_key[i]);
        out_parent[(size_t)b * k + i] = b * beams_in + win_idx[i] / n;
    }
}

// The exact step (rqhip_beam_topk_step): every code of every row is a candidate, nothing is drawn.  beams_in * K keys do
// not fit in LDS and need not: under the total order (score descending, then j = beam * K + c ascending) the k best of
// a user lie among the m = min(k, K) best of each row.
//
//   phase A (one wave per row, rows strided over the waves): lp[c] = (x[c] - max) - logf(sum expf(x - max)) in fp32,
//            score = lp[c] (+ the parent beam's score when h > 0), NaN -> -inf; a code whose (h+1)-prefix is not in the
//            corpus scores -inf: the parent prefix is hashed once per row, then one sid_hash_step and one probe per
//            code.  The order images go into the wave's [K] slice and wave_top takes the m best, ties to the lower code:
//            candidate beam * m + rank, which orders equal scores exactly as beam * K + c does.
//   phase B (wave 0): the k best of the beams_in * m candidates, ties (-inf included) to the lower candidate.
//   phase C (all threads): ids = parent ids ++ code, scores, the global parent row.
//
// wave_top's two preconditions hold by construction: no key is 0 (a NaN is made -inf BEFORE f32_order, which maps
// every other value above 0), and it is never asked for more keys than its slice holds (m <= K, k <= beams_in * m).
__global__ __launch_bounds__(256) void beam_topk_step_kernel(
    const float *__restrict__ logits, long long ld_logits, const float *__restrict__ parent_scores,
    const int64_t *__restrict__ parent_ids, int h, int beams_in, int K, int m, int k, const int *__restrict__ table,
    unsigned mask, const int64_t *__restrict__ corpus, long long N, long long ld, int64_t *__restrict__ out_ids,
    float *__restrict__ out_scores, int64_t *__restrict__ out_parent) {
    extern __shared__ unsigned lds[];
    __shared__ int win_idx[kBeamMaxTopK];
    __shared__ unsigned win_key[kBeamMaxTopK];

    const int nw = blockDim.x / RQ_WAVE;
    const int wave = threadIdx.x / RQ_WAVE, lane = threadIdx.x & (RQ_WAVE - 1);
    const long long b = blockIdx.x;
    const int C = beams_in * m;
    unsigned *rowkeys = lds + (size_t)wave * K;      // [K] per wave
    unsigned *ckey = lds + (size_t)nw * K;           // [C] order image of each candidate's score
    int *ccode = reinterpret_cast<int *>(ckey + C);  // [C] code of each candidate

    const unsigned neg_inf = f32_order(-INFINITY);
    const size_t slots = (size_t)mask + 1;
    const int *tab = table + (size_t)h * slots;

    // ---- phase A: log-softmax, validity of every code, the m best of the row
    for (int beam = wave; beam < beams_in; beam += nw) {
        const long long row = b * beams_in + beam;
        const float *x = logits + (size_t)row * (size_t)ld_logits;
        float mx = -INFINITY;
        for (int c = lane; c < K; c += RQ_WAVE) mx = fmaxf(mx, x[c]);
        mx = wave_max_f32(mx);
        float s = 0.f;
        for (int c = lane; c < K; c += RQ_WAVE) s += expf(x[c] - mx);
        s = wave_sum_f32(s);
        const float ls = logf(s);
        const bool add_base = parent_scores != nullptr;
        const float base = add_base ? parent_scores[row] : 0.f;
        const int64_t *par = parent_ids + (size_t)row * (size_t)h;  // not read when h == 0
        unsigned hpar = kSidHashSeed;
        for (int t = 0; t < h; ++t) hpar = sid_hash_step(hpar, par[t]);
        for (int c = lane; c < K; c += RQ_WAVE) {
            float sc = (x[c] - mx) - ls;
            if (add_base) sc = sc + base;
            if (!(sc == sc)) sc = -INFINITY;  // NaN: its all-ones pattern would map to the retired mark
            unsigned key = f32_order(sc);
            if (key != neg_inf) {
                bool found = false;
                if (N > 0) {
                    unsigned slot = sid_hash_final(sid_hash_step(hpar, (int64_t)c)) & mask;
                    for (;;) {
                        const int prev = tab[slot];
                        if (prev == -1) break;
                        const int64_t *other = corpus + (size_t)prev * (size_t)ld;
                        bool same = other[h] == (int64_t)c;
                        for (int t = 0; t < h && same; ++t) same = other[t] == par[t];
                        if (same) {
                            found = true;
                            break;
                        }
                        slot = (slot + 1) & mask;
                    }
                }
                if (!found) key = neg_inf;
            }
            rowkeys[c] = key;
        }
        wave_top(rowkeys, K, m, lane, [&](int r, int c, unsigned v) {
            ckey[beam * m + r] = v;
            ccode[beam * m + r] = c;
        });
    }
    __syncthreads();

    // ---- phase B: the k best candidates of the user
    if (wave == 0) {
        wave_top(ckey, C, k, lane, [&](int r, int j, unsigned v) {
            win_idx[r] = j;
            win_key[r] = v;
        });
    }
    __syncthreads();

    // ---- phase C: outputs
    const int h1 = h + 1;
    for (int e = threadIdx.x; e < k * h1; e += blockDim.x) {
        const int i = e / h1, t = e - i * h1;
        const int j = win_idx[i];
        const int beam = j / m;
        const int64_t v = t < h ? parent_ids[((size_t)b * beams_in + beam) * (size_t)h + t] : (int64_t)ccode[j];
        out_ids[((size_t)b * k + i) * (size_t)h1 + t] = v;
    }
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        out_scores[(size_t)b * k + i] = f32_from_order(win_key[i]);
        out_parent[(size_t)b * k + i] = b * beams_in + win_idx[i] / m;
    }
}

int beam_waves(int beams_in) { return beams_in < kBeamMaxWaves ? beams_in : kBeamMaxWaves; }

int topk_keep(int K, int k) { return k < K ? k : K; }  // candidates kept per row

size_t topk_lds_bytes(int beams_in, int K, int k) {
    return ((size_t)beam_waves(beams_in) * (size_t)K + 2 * (size_t)beams_in * (size_t)topk_keep(K, k)) * sizeof(unsigned);
}

int check_topk_args(int64_t B, int beams_in, int K, int k, int h) {
    if (B < 0 || beams_in < 1 || K < 1 || k < 1 || h < 0) {
        set_error("beam_topk_step: bad sizes (B=%lld, beams_in=%d, K=%d, k=%d, h=%d)", (long long)B, beams_in, K, k, h);
        return RQHIP_EARG;
    }
    if (h == 0 && beams_in != 1) {
        set_error("beam_topk_step: h = 0 takes beams_in = 1 (got %d)", beams_in);
        return RQHIP_EARG;
    }
    if ((long long)k > (long long)beams_in * (long long)K) {
        set_error("beam_topk_step: k=%d exceeds the beams_in * K = %lld candidates", k, (long long)beams_in * K);
        return RQHIP_EARG;
    }
    if (K > kBeamMaxK) {
        set_error("beam_topk_step: K=%d exceeds K <= %d", K, kBeamMaxK);
        return RQHIP_EUNSUPPORTED;
    }
    if (k > kBeamMaxTopK) {
        set_error("beam_topk_step: k=%d exceeds k <= %d", k, kBeamMaxTopK);
        return RQHIP_EUNSUPPORTED;
    }
    if (beams_in > kBeamMaxTopK) {
        set_error("beam_topk_step: beams_in=%d exceeds beams_in <= %d", beams_in, kBeamMaxTopK);
        return RQHIP_EUNSUPPORTED;
    }
    if (h + 1 > RQHIP_MAX_PREFIX_LEN) {
        set_error("beam_topk_step: h + 1 = %d exceeds h + 1 <= RQHIP_MAX_PREFIX_LEN = %d", h + 1, RQHIP_MAX_PREFIX_LEN);
        return RQHIP_EUNSUPPORTED;
    }
    if (B >= (1ll << 31)) {
        set_error("beam_topk_step: B=%lld exceeds one workgroup per user (B < 2^31)", (long long)B);
        return RQHIP_EUNSUPPORTED;
    }
    return RQHIP_OK;
}

size_t beam_lds_bytes(int beams_in, int K, int n) {
    return ((size_t)beam_waves(beams_in) * (size_t)K + 2 * (size_t)beams_in * (size_t)n) * sizeof(unsigned);
}

int check_beam_args(int64_t B, int beams_in, int K, int n_cands, int k, int h) {
    if (B < 0 || beams_in < 1 || K < 1 || n_cands < 1 || k < 1 || h < 0) {
        set_error("beam_step: bad sizes (B=%lld, beams_in=%d, K=%d, n_cands=%d, k=%d, h=%d)", (long long)B, beams_in, K,
                  n_cands, k, h);
        return RQHIP_EARG;
    }
    if (h == 0 && beams_in != 1) {
        set_error("beam_step: h = 0 takes beams_in = 1 (got %d)", beams_in);
        return RQHIP_EARG;
    }
    if (n_cands > K) {
        set_error("beam_step: n_cands=%d exceeds K=%d (sampling without replacement)", n_cands, K);
        return RQHIP_EARG;
    }
    if (k > beams_in * n_cands) {
        set_error("beam_step: k=%d exceeds the beams_in * n_cands = %d candidates", k, beams_in * n_cands);
        return RQHIP_EARG;
    }
    if (K > kBeamMaxK) {
        set_error("beam_step: K=%d exceeds K <= %d", K, kBeamMaxK);
        return RQHIP_EUNSUPPORTED;
    }
    if (n_cands > kBeamMaxCands) {
        set_error("beam_step: n_cands=%d exceeds n_cands <= %d", n_cands, kBeamMaxCands);
        return RQHIP_EUNSUPPORTED;
    }
    if (k > kBeamMaxTopK || beams_in > kBeamMaxTopK) {
        set_error("beam_step: k=%d / beams_in=%d exceed k <= %d", k, beams_in, kBeamMaxTopK);
        return RQHIP_EUNSUPPORTED;
    }
    if (h + 1 > RQHIP_MAX_PREFIX_LEN) {
        set_error("beam_step: h + 1 = %d exceeds h + 1 <= RQHIP_MAX_PREFIX_LEN = %d", h + 1, RQHIP_MAX_PREFIX_LEN);
        return RQHIP_EUNSUPPORTED;
    }
    if (B >= (1ll << 31)) {
        set_error("beam_step: B=%lld exceeds one workgroup per user (B < 2^31)", (long long)B);
        return RQHIP_EUNSUPPORTED;
    }
    return RQHIP_OK;
}

}  // namespace

}  // namespace rqhip

using namespace rqhip;

extern "C" size_t rqhip_beam_step_workspace_bytes(int64_t B, int beams_in, int K, int n_cands, int k) {
    (void)B, (void)beams_in, (void)K, (void)n_cands, (void)k;
    return 0;  // everything lives in LDS; the argument is kept so callers need not change if that ever does
}

extern "C" int rqhip_beam_step(const float *logits, int64_t ld_logits, const float *noise, const float *parent_scores,
                               const int64_t *parent_ids, int h, int64_t B, int beams_in, int K, int n_cands, int k,
                               const void *index, size_t index_bytes, const int64_t *corpus, int64_t N, int H,
                               int64_t ld, int64_t *out_ids, float *out_scores, int64_t *out_parent, void *workspace,
                               size_t workspace_bytes, rqhip_stream_t stream) {
    if (int rc = check_beam_args(B, beams_in, K, n_cands, k, h)) return rc;
    if (N < 0 || H < 1 || H > RQHIP_MAX_PREFIX_LEN || ld < H || (N > 0 && !corpus)) {
        set_error("beam_step: bad corpus (N=%lld, H=%d, ld=%lld; 1 <= H <= %d, ld >= H)", (long long)N, H,
                  (long long)ld, RQHIP_MAX_PREFIX_LEN);
        return RQHIP_EARG;
    }
    if (N >= (1ll << 30)) {
        set_error("beam_step: N=%lld exceeds the 2^30 rows the prefix index holds", (long long)N);
        return RQHIP_EUNSUPPORTED;
    }
    if (h + 1 > H) {
        set_error("beam_step: prefix length h + 1 = %d exceeds the corpus' H = %d id levels", h + 1, H);
        return RQHIP_EARG;
    }
    if (ld_logits < K) {
        set_error("beam_step: ld_logits=%lld < K=%d", (long long)ld_logits, K);
        return RQHIP_EARG;
    }
    if (B > 0 && (!logits || !noise || !out_ids || !out_scores || !out_parent ||
                  (h > 0 && (!parent_scores || !parent_ids)))) {
        set_error("beam_step: null pointer (logits, noise, outputs; parent_scores / parent_ids when h > 0)");
        return RQHIP_EARG;
    }
    if (!index || index_bytes < rqhip_prefix_index_bytes(N, H)) {
        set_error("beam_step: index buffer too small for N=%lld, H=%d", (long long)N, H);
        return RQHIP_EWORKSPACE;
    }
    if (workspace_bytes < rqhip_beam_step_workspace_bytes(B, beams_in, K, n_cands, k)) {
        set_error("beam_step: workspace too small");
        return RQHIP_EWORKSPACE;
    }
    (void)workspace;
    if (B == 0) return RQHIP_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = beam_lds_bytes(beams_in, K, n_cands);
    if (lds > 64 * 1024) {
        static LdsGrant grant;
        RQ_RETURN_IF_HIP(grant.ensure(reinterpret_cast<const void *>(beam_step_kernel), (int)lds));
    }
    hipLaunchKernelGGL(beam_step_kernel, dim3((unsigned)B), dim3(RQ_WAVE * beam_waves(beams_in)), lds, s, logits,
                       (long long)ld_logits, noise, h > 0 ? parent_scores : nullptr, h > 0 ? parent_ids : nullptr, h,
                       beams_in, K, n_cands, k, reinterpret_cast<const int *>(index), (unsigned)(slots_for(N) - 1),
                       corpus, (long long)N, (long long)ld, out_ids, out_scores, out_parent);
    RQ_CHECK_LAUNCH("beam_step_kernel");
    return RQHIP_OK;
}

extern "C" int rqhip_beam_topk_step(const float *logits, int64_t ld_logits, const float *parent_scores,
                                    const int64_t *parent_ids, int h, int64_t B, int beams_in, int K, int k,
                                    const void *index, size_t index_bytes, const int64_t *corpus, int64_t N, int H,
                                    int64_t ld, int64_t *out_ids, float *out_scores, int64_t *out_parent,
                                    rqhip_stream_t stream) {
    if (int rc = check_topk_args(B, beams_in, K, k, h)) return rc;
    if (N < 0 || H < 1 || H > RQHIP_MAX_PREFIX_LEN || ld < H || (N > 0 && !corpus)) {
        set_error("beam_topk_step: bad corpus (N=%lld, H=%d, ld=%lld; 1 <= H <= %d, ld >= H)", (long long)N, H,
                  (long long)ld, RQHIP_MAX_PREFIX_LEN);
        return RQHIP_EARG;
    }
    if (N >= (1ll << 30)) {
        set_error("beam_topk_step: N=%lld exceeds the 2^30 rows the prefix index holds", (long long)N);
        return RQHIP_EUNSUPPORTED;
    }
    if (h + 1 > H) {
        set_error("beam_topk_step: prefix length h + 1 = %d exceeds the corpus' H = %d id levels", h + 1, H);
        return RQHIP_EARG;
    }
    if (ld_logits < K) {
        set_error("beam_topk_step: ld_logits=%lld < K=%d", (long long)ld_logits, K);
        return RQHIP_EARG;
    }
    if (B > 0 && (!logits || !out_ids || !out_scores || !out_parent || (h > 0 && (!parent_scores || !parent_ids)))) {
        set_error("beam_topk_step: null pointer (logits, outputs; parent_scores / parent_ids when h > 0)");
        return RQHIP_EARG;
    }
    if (!index || index_bytes < rqhip_prefix_index_bytes(N, H)) {
        set_error("beam_topk_step: index buffer too small for N=%lld, H=%d", (long long)N, H);
        return RQHIP_EWORKSPACE;
    }
    if (B == 0) return RQHIP_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = topk_lds_bytes(beams_in, K, k);
    if (lds > 64 * 1024) {
        static LdsGrant grant;
        RQ_RETURN_IF_HIP(grant.ensure(reinterpret_cast<const void *>(beam_topk_step_kernel), (int)lds));
    }
    hipLaunchKernelGGL(beam_topk_step_kernel, dim3((unsigned)B), dim3(RQ_WAVE * beam_waves(beams_in)), lds, s, logits,
                       (long long)ld_logits, h > 0 ? parent_scores : nullptr, h > 0 ? parent_ids : nullptr, h, beams_in,
                       K, topk_keep(K, k), k, reinterpret_cast<const int *>(index), (unsigned)(slots_for(N) - 1), corpus,
                       (long long)N, (long long)ld, out_ids, out_scores, out_parent);
    RQ_CHECK_LAUNCH("beam_topk_step_kernel");
    return RQHIP_OK;
}

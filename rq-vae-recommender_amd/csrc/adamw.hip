// adamw.hip -- the AdamW update of every parameter of the model in ONE launch (gfx950).  Reference: train_rqvae.py:136-138
// (`AdamW(params=model.parameters(), lr, weight_decay)`: decoupled weight decay on every parameter, codebooks included; SURVEY.md
// appendix A item 16).
//
// Why not torch's fused AdamW: its multi-tensor kernel hands 64 K-element chunks to workgroups -- 1.15 M parameters are 18 chunks, 18 of
// 256 CUs work, 40-46 us per step at every batch size (11 % of the 0.35 ms hipGraph step at batch 640, 1.6 % at 100 000 rows), plus a
// second launch that increments the per-parameter step counters.  Here: 1024 elements per workgroup (1 100 workgroups); the step counter is a
// device scalar (so a captured hipGraph advances it on replay), bumped by a one-thread kernel that also forms the bias corrections.
// The arithmetic is torch's `_fused_adamw_` (aten/src/ATen/native/cuda/fused_adam_utils.cuh, ADAMW mode, no amsgrad, no maximize), in fp32:
//     p  -= lr wd p
//     m   = lerp(m, g, 1 - b1)              (= m + (1 - b1) (g - m) for 1 - b1 < 0.5)
//     v   = b2 v + (1 - b2) g g
//     p  -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps),          t = step + 1
// -- the same update as the reference's (foreach) AdamW up to the rounding of each operation (tests/test_gpu_optim.py holds both to 1e-6).
#include <math.h>

#include "rqhip_common.h"

namespace rqhip {

typedef float aw_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kAwMaxJobs = 24;
constexpr int kAwBlockElems = 1024;      // 256 threads x one float4

struct AdamwJob {
    float *p, *m, *v;
    const float *g;
    long long n;
    int block0;
};
struct AdamwJobs {
    AdamwJob j[kAwMaxJobs];
    int n;
};

// step += 1 and the scalars every element needs, once per step, by one thread -- so that the update kernel only READS them (a first version
// let every workgroup read the counter and the last one to finish bump it: 1 100 returning atomics on one word are 13 us by themselves, and
// every thread evaluated two powf)
struct AdamwScalars {
    float step_size, bc2_sqrt;
};
__global__ void adamw_bump_kernel(float *__restrict__ step, AdamwScalars *__restrict__ sc, float lr, float beta1, float beta2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float t = step[0] + 1.0f;
    step[0] = t;
    const float bc1 = 1.0f - powf(beta1, t), bc2 = 1.0f - powf(beta2, t);
    sc->step_size = lr / bc1;
    sc->bc2_sqrt = sqrtf(bc2);
}

__global__ __launch_bounds__(256) void adamw_kernel(const AdamwJobs jobs, const AdamwScalars *__restrict__ sc, float lr, float beta1, float beta2,
                                                    float eps, float wd) {
    AdamwJob job = jobs.j[0];
#pragma unroll
    for (int i = 1; i < kAwMaxJobs; ++i)
        if (i < jobs.n && (int)blockIdx.x >= jobs.j[i].block0) job = jobs.j[i];
    const float step_size = sc->step_size, bc2_sqrt = sc->bc2_sqrt;
    const long long i0 = ((long long)((int)blockIdx.x - job.block0) * 256 + threadIdx.x) * 4;
    auto one = [&](float &p, float &m, float &v, float g) {
        p = p - (lr * wd) * p;
        m = m + (1.0f - beta1) * (g - m);
        v = beta2 * v + ((1.0f - beta2) * g) * g;
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        p = p - step_size * (m / denom);
    };
    if (i0 + 3 < job.n) {
        aw_f32x4 p = *reinterpret_cast<aw_f32x4 *>(job.p + i0), m = *reinterpret_cast<aw_f32x4 *>(job.m + i0);
        aw_f32x4 v = *reinterpret_cast<aw_f32x4 *>(job.v + i0);
        const aw_f32x4 g = *reinterpret_cast<const aw_f32x4 *>(job.g + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = p[k], mk = m[k], vk = v[k];
            one(pk, mk, vk, g[k]);
            p[k] = pk; m[k] = mk; v[k] = vk;
        }
        *reinterpret_cast<aw_f32x4 *>(job.p + i0) = p;
        *reinterpret_cast<aw_f32x4 *>(job.m + i0) = m;
        *reinterpret_cast<aw_f32x4 *>(job.v + i0) = v;
    } else {
        for (long long i = i0; i < job.n; ++i) one(job.p[i], job.m[i], job.v[i], job.g[i]);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The optimizer tail of the retrieval model's training loop (reference train_decoder.py:147-151, 202-205: `clip_grad_norm_`, AdamW,
// `InverseSquareRootScheduler.step()`) with every scalar of it formed ON THE DEVICE, so that a captured hipGraph replays a step whose
// clip coefficient and learning rate are this step's, not the capture's:
//     adamw_sumsq_kernel     one fp32 partial sum of g^2 per workgroup, over the element range the update gives that workgroup; stored,
//                            not added atomically: the norm is the same bits on every run
//     adamw_tail_scalars_kernel   ONE workgroup: the partials summed in a fixed order (in double: 256 threads, a handful of terms each),
//                            norm, clip coefficient, t += 1, the scheduled lr from the device counter lr_step (then lr_step += 1), and the
//                            two bias-correction scalars of adamw_bump_kernel from that lr
//     adamw_tail_kernel      adamw_kernel's element arithmetic on g * coef, lr read from the scalars; gradients are not written back
// Job tables travel BY VALUE in the kernel-argument segment (4 KB): 64 tensors per update launch (44 bytes each), 128 per sum-of-squares
// launch (20 bytes each) -- the retrieval model's ~95 tensors are 1 + 1 + 2 launches.  A device-resident table would make it 1 + 1 + 1, but
// it has to be uploaded again whenever a gradient pointer changes (autograd allocates new gradients after every zero_grad(set_to_none)),
// and an upload cannot be issued under stream capture; by-value arguments are captured with the launch.  With more than 24 entries the
// workgroup finds its job by binary search over the first-workgroup indices (uniform: scalar loads from the argument segment) instead
// of adamw_kernel's unrolled select.
constexpr int kTailJobs = 64;
constexpr int kSumsqJobs = 128;
constexpr int kTailThreads = 256;

struct TailJobs {            // struct of arrays: the lookup touches block0[] only
    float *p[kTailJobs], *m[kTailJobs], *v[kTailJobs];
    const float *g[kTailJobs];
    long long n[kTailJobs];
    int block0[kTailJobs];
    int count;
};
struct SumsqJobs {
    const float *g[kSumsqJobs];
    long long n[kSumsqJobs];
    int block0[kSumsqJobs];
    int count;
    int part0;               // index of this launch's first partial
};
static_assert(sizeof(TailJobs) + 64 <= 4096 && sizeof(SumsqJobs) + 64 <= 4096, "job tables must fit the kernel-argument segment");

// what rqhip_adamw_tail_step leaves in `scalars` (RQHIP_ADAMW_TAIL_SCALARS floats)
struct TailScalars {
    float step_size, bc2_sqrt;      // as AdamwScalars
    float lr, coef, norm;
    float pad[3];
};
static_assert(sizeof(TailScalars) == RQHIP_ADAMW_TAIL_SCALARS * sizeof(float), "include/rqhip.h describes this layout");

// the last i in [0, count) with block0[i] <= b (block0[0] == 0, ascending)
template <int N>
__device__ __forceinline__ int tail_find_job(const int (&block0)[N], int count, int b) {
    int lo = 0, hi = count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (block0[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kTailThreads) void adamw_sumsq_kernel(const SumsqJobs jobs, float *__restrict__ partials) {
    __shared__ float wave_sum[kTailThreads / RQ_WAVE];
    const int b = (int)blockIdx.x;
    const int j = tail_find_job(jobs.block0, jobs.count, b);
    const float *__restrict__ g = jobs.g[j];
    const long long n = jobs.n[j];
    const long long i0 = ((long long)(b - jobs.block0[j]) * kTailThreads + threadIdx.x) * 4;
    float s = 0.0f;
    if (i0 + 3 < n) {
        const aw_f32x4 x = *reinterpret_cast<const aw_f32x4 *>(g + i0);
        s = x[0] * x[0];
        s = s + x[1] * x[1];
        s = s + x[2] * x[2];
        s = s + x[3] * x[3];
    } else {
        for (long long i = i0; i < n; ++i) s = s + g[i] * g[i];
    }
#pragma unroll
    for (int off = RQ_WAVE / 2; off > 0; off >>= 1) s = s + __shfl_xor(s, off, RQ_WAVE);
    if ((threadIdx.x & (RQ_WAVE - 1)) == 0) wave_sum[threadIdx.x / RQ_WAVE] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[jobs.part0 + b] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// max_norm <= 0: no clipping (coef 1, norm NaN = not computed; n_partials is 0).  warmup < 0: no schedule (lr = the argument, lr_step untouched).
__global__ __launch_bounds__(kTailThreads) void adamw_tail_scalars_kernel(float *__restrict__ step, long long *__restrict__ lr_step,
                                                                          TailScalars *__restrict__ sc, const float *__restrict__ partials,
                                                                          long long n_partials, float max_norm, float lr_arg, double base_lr,
                                                                          long long warmup, float beta1, float beta2) {
    __shared__ double wave_sum[kTailThreads / RQ_WAVE];
    double acc = 0.0;
    if (max_norm > 0.0f) {
        for (long long i = threadIdx.x; i < n_partials; i += kTailThreads) acc += (double)partials[i];
#pragma unroll
        for (int off = RQ_WAVE / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, RQ_WAVE);
        if ((threadIdx.x & (RQ_WAVE - 1)) == 0) wave_sum[threadIdx.x / RQ_WAVE] = acc;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float norm = __builtin_nanf(""), coef = 1.0f;
    if (max_norm > 0.0f) {
        norm = (float)sqrt((wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]));
        const float c = max_norm / (norm + 1e-6f);      // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1)
        coef = c > 1.0f ? 1.0f : c;                     // (a NaN stays a NaN, as under torch.clamp)
    }
    float lr = lr_arg;
    if (warmup >= 0) {
        const long long ls = lr_step[0];
        lr_step[0] = ls + 1;
        const double lr_d = ls <= warmup ? base_lr : base_lr * (sqrt((double)warmup) / sqrt((double)ls));
        lr = (float)lr_d;
    }
    const float t = step[0] + 1.0f;
    step[0] = t;
    const float bc1 = 1.0f - powf(beta1, t), bc2 = 1.0f - powf(beta2, t);
    sc->step_size = lr / bc1;
    sc->bc2_sqrt = sqrtf(bc2);
    sc->lr = lr;
    sc->coef = coef;
    sc->norm = norm;
}

__global__ __launch_bounds__(kTailThreads) void adamw_tail_kernel(const TailJobs jobs, const TailScalars *__restrict__ sc, float beta1, float beta2,
                                                                  float eps, float wd) {
    const int b = (int)blockIdx.x;
    const int j = tail_find_job(jobs.block0, jobs.count, b);
    float *__restrict__ jp = jobs.p[j], *__restrict__ jm = jobs.m[j], *__restrict__ jv = jobs.v[j];
    const float *__restrict__ jg = jobs.g[j];
    const long long n = jobs.n[j];
    const float step_size = sc->step_size, bc2_sqrt = sc->bc2_sqrt, lr = sc->lr, coef = sc->coef;
    const long long i0 = ((long long)(b - jobs.block0[j]) * kTailThreads + threadIdx.x) * 4;
    auto one = [&](float &p, float &m, float &v, float g_raw) {
        const float g = g_raw * coef;
        p = p - (lr * wd) * p;
        m = m + (1.0f - beta1) * (g - m);
        v = beta2 * v + ((1.0f - beta2) * g) * g;
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        p = p - step_size * (m / denom);
    };
    if (i0 + 3 < n) {
        aw_f32x4 p = *reinterpret_cast<aw_f32x4 *>(jp + i0), m = *reinterpret_cast<aw_f32x4 *>(jm + i0);
        aw_f32x4 v = *reinterpret_cast<aw_f32x4 *>(jv + i0);
        const aw_f32x4 g = *reinterpret_cast<const aw_f32x4 *>(jg + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = p[k], mk = m[k], vk = v[k];
            one(pk, mk, vk, g[k]);
            p[k] = pk; m[k] = mk; v[k] = vk;
        }
        *reinterpret_cast<aw_f32x4 *>(jp + i0) = p;
        *reinterpret_cast<aw_f32x4 *>(jm + i0) = m;
        *reinterpret_cast<aw_f32x4 *>(jv + i0) = v;
    } else {
        for (long long i = i0; i < n; ++i) one(jp[i], jm[i], jv[i], jg[i]);
    }
}

// workgroups (= partials) of the tensors numel[0..n); -1 and an error message for an invalid list
static long long tail_blocks(const int64_t *numel, int n, const char *who) {
    if (n < 0 || (n > 0 && !numel)) {
        set_error("%s: negative count or null numel", who);
        return -1;
    }
    long long blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0) {
            set_error("%s: tensor %d: negative numel", who, i);
            return -1;
        }
        blocks += (numel[i] + kAwBlockElems - 1) / kAwBlockElems;
        if (blocks > 0x7fffffffLL) {
            set_error("%s: more than 2^31 - 1 workgroups", who);
            return -1;
        }
    }
    return blocks;
}

}  // namespace rqhip

using namespace rqhip;

// One AdamW step over n tensors: p[i] (updated in place), g[i], m[i], v[i] of numel[i] fp32 elements each (16-byte aligned, contiguous).
// `step`: device float scalar, the number of steps taken so far (incremented by the call); `scratch`: 8 device bytes the call may overwrite.
extern "C" int rqhip_adamw_step(float *const *p, const float *const *g, float *const *m, float *const *v, const int64_t *numel, int n,
                                float *step, unsigned *scratch, float lr, float beta1, float beta2, float eps, float weight_decay,
                                rqhip_stream_t stream) {
    if (n < 0 || !step || !scratch || (n > 0 && (!p || !g || !m || !v || !numel))) {
        set_error("adamw_step: null pointer");
        return RQHIP_EARG;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    auto al16 = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; };
    AdamwScalars *sc = reinterpret_cast<AdamwScalars *>(scratch);
    hipLaunchKernelGGL(adamw_bump_kernel, dim3(1), dim3(64), 0, s, step, sc, lr, beta1, beta2);
    RQ_CHECK_LAUNCH("adamw_bump_kernel");
    int first = 0;
    while (first < n) {      // launches of at most kAwMaxJobs tensors (empty tensors are skipped)
        AdamwJobs jobs;
        jobs.n = 0;
        int blocks = 0, i = first;
        for (; i < n && jobs.n < kAwMaxJobs; ++i) {
            if (numel[i] <= 0) continue;
            if (!p[i] || !g[i] || !m[i] || !v[i] || !al16(p[i]) || !al16(g[i]) || !al16(m[i]) || !al16(v[i])) {
                set_error("adamw_step: tensor %d: null or not 16-byte aligned", i);
                return RQHIP_EARG;
            }
            AdamwJob &j = jobs.j[jobs.n++];
            j.p = p[i]; j.g = g[i]; j.m = m[i]; j.v = v[i]; j.n = numel[i]; j.block0 = blocks;
            blocks += (int)((numel[i] + kAwBlockElems - 1) / kAwBlockElems);
        }
        if (jobs.n > 0) {
            hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, s, jobs, sc, lr, beta1, beta2, eps, weight_decay);
            RQ_CHECK_LAUNCH("adamw_kernel");
        }
        first = i;
    }
    return RQHIP_OK;
}

// Bytes of `workspace` rqhip_adamw_tail_step needs for these tensors (one fp32 partial per 1024 elements of every tensor); no GPU needed.
extern "C" int64_t rqhip_adamw_tail_workspace_bytes(const int64_t *numel, int n) {
    const long long blocks = tail_blocks(numel, n, "adamw_tail_workspace_bytes");
    return blocks < 0 ? -1 : (int64_t)(blocks * (long long)sizeof(float));
}

// Clip by the global 2-norm, scheduled learning rate and AdamW over n tensors, every scalar formed on the device (see the kernels above).
extern "C" int rqhip_adamw_tail_step(float *const *p, const float *const *g, float *const *m, float *const *v, const int64_t *numel, int n,
                                     float *step, int64_t *lr_step, float *scalars, float *workspace, size_t workspace_bytes,
                                     float max_norm, float lr, double base_lr, int64_t warmup, float beta1, float beta2, float eps,
                                     float weight_decay, rqhip_stream_t stream) {
    // every argument is checked before the first launch
    if (n < 0 || !step || !scalars || (n > 0 && (!p || !g || !m || !v || !numel))) {
        set_error("adamw_tail_step: null pointer or negative count");
        return RQHIP_EARG;
    }
    auto al16 = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; };
    if (!al16(scalars) || (reinterpret_cast<uintptr_t>(step) & 3u) || (reinterpret_cast<uintptr_t>(lr_step) & 7u)) {
        set_error("adamw_tail_step: scalars must be 16-byte aligned, step 4-byte, lr_step 8-byte");
        return RQHIP_EARG;
    }
    if (warmup >= 0 && !lr_step) {
        set_error("adamw_tail_step: a schedule (warmup >= 0) needs lr_step");
        return RQHIP_EARG;
    }
    const long long blocks = tail_blocks(numel, n, "adamw_tail_step");
    if (blocks < 0) return RQHIP_EARG;
    for (int i = 0; i < n; ++i) {
        if (numel[i] == 0) continue;
        if (!p[i] || !g[i] || !m[i] || !v[i] || !al16(p[i]) || !al16(g[i]) || !al16(m[i]) || !al16(v[i])) {
            set_error("adamw_tail_step: tensor %d: null or not 16-byte aligned", i);
            return RQHIP_EARG;
        }
    }
    const bool clip = max_norm > 0.0f;
    if (clip && blocks > 0 && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 3u) || workspace_bytes < (size_t)blocks * sizeof(float))) {
        set_error("adamw_tail_step: workspace null, misaligned or smaller than rqhip_adamw_tail_workspace_bytes (%lld)",
                  blocks * (long long)sizeof(float));
        return RQHIP_EARG;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (clip) {
        int first = 0, part0 = 0;
        while (first < n) {      // launches of at most kSumsqJobs tensors (empty tensors are skipped)
            SumsqJobs jobs;
            jobs.count = 0;
            jobs.part0 = part0;
            int launch_blocks = 0, i = first;
            for (; i < n && jobs.count < kSumsqJobs; ++i) {
                if (numel[i] == 0) continue;
                const int k = jobs.count++;
                jobs.g[k] = g[i]; jobs.n[k] = numel[i]; jobs.block0[k] = launch_blocks;
                launch_blocks += (int)((numel[i] + kAwBlockElems - 1) / kAwBlockElems);
            }
            if (jobs.count > 0) {
                hipLaunchKernelGGL(adamw_sumsq_kernel, dim3((unsigned)launch_blocks), dim3(kTailThreads), 0, s, jobs, workspace);
                RQ_CHECK_LAUNCH("adamw_sumsq_kernel");
            }
            part0 += launch_blocks;
            first = i;
        }
    }
    TailScalars *sc = reinterpret_cast<TailScalars *>(scalars);
    hipLaunchKernelGGL(adamw_tail_scalars_kernel, dim3(1), dim3(kTailThreads), 0, s, step, reinterpret_cast<long long *>(lr_step), sc, workspace,
                       clip ? blocks : 0LL, max_norm, lr, base_lr, (long long)warmup, beta1, beta2);
    RQ_CHECK_LAUNCH("adamw_tail_scalars_kernel");
    int first = 0;
    while (first < n) {          // launches of at most kTailJobs tensors
        TailJobs jobs;
        jobs.count = 0;
        int launch_blocks = 0, i = first;
        for (; i < n && jobs.count < kTailJobs; ++i) {
            if (numel[i] == 0) continue;
            const int k = jobs.count++;
            jobs.p[k] = p[i]; jobs.g[k] = g[i]; jobs.m[k] = m[i]; jobs.v[k] = v[i]; jobs.n[k] = numel[i]; jobs.block0[k] = launch_blocks;
            launch_blocks += (int)((numel[i] + kAwBlockElems - 1) / kAwBlockElems);
        }
        if (jobs.count > 0) {
            hipLaunchKernelGGL(adamw_tail_kernel, dim3((unsigned)launch_blocks), dim3(kTailThreads), 0, s, jobs, sc, beta1, beta2, eps, weight_decay);
            RQ_CHECK_LAUNCH("adamw_tail_kernel");
        }
        first = i;
    }
    return RQHIP_OK;
}

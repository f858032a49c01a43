// t5_images.hip -- bf16 weight images for the "bf16" arithmetic of t5_ffn.hip and t5_proj.hip (gfx950; modules/t5.py,
// weight_images = "bf16"; semantics in include/rqhip.h).  The image of a row-major fp32 matrix is the same matrix with
// every element rounded to bf16 by the conversion csrc/t5_common.h:pack_bf16x8 uses, so an image element is the very
// operand the bf16 kernels would form in registers; the transposed image holds the same bits the other way round, so
// that a backward kernel too reads its reduction terms along rows.
//
// One launch serves any number of matrices.  The job table lives in device memory (the caller builds it once and
// rebuilds it only when a pointer changes), so a refresh is one kernel launch and nothing else.  Every job carries the
// number of tiles of the jobs before it; workgroup b owns tile b of the concatenation and finds its job by bisection of
// those prefix sums (csrc/wgrad_jobs.hip keeps its table by value and scans it; this table has no size limit).
//
// A workgroup of 256 threads owns one 32 x 32 tile (rows and columns are multiples of 32: every tile is full).  Thread
// (r, c4) = (t >> 3, t & 7) loads the float4 at row r, columns 4 c4 .. 4 c4 + 3: a row's 128 bytes are contiguous.  It
// stores its 4 rounded elements to the image (64 contiguous bytes per row) and into an LDS tile; after the barrier it
// is thread (c, r4) of the transposed tile and stores elements 4 r4 .. 4 r4 + 3 of row c of the transposed image.
#include "rqhip_common.h"
#include "t5_common.h"

namespace rqhip {

namespace {

constexpr int kImgTile = 32;
constexpr int kImgLd = kImgTile + 2;      // LDS row stride in elements: an odd number of words

struct ImgJob {
    const float *src;       // [rows, cols]
    __bf16 *img;            // [rows, cols]
    __bf16 *img_t;          // [cols, rows], or null
    int rows, cols;
    long long tile0;        // tiles of the jobs before this one
};
static_assert(sizeof(ImgJob) == 40, "the job table's layout is part of rqhip_bf16_images_job_bytes");

__global__ __launch_bounds__(256) void t5_bf16_images_kernel(const ImgJob *__restrict__ jobs, int n_jobs) {
    __shared__ __bf16 tile[kImgTile * kImgLd];
    const long long b = blockIdx.x;
    int lo = 0, hi = n_jobs;          // the last job whose first tile is at or before b: tile0 ascends strictly
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].tile0 <= b) lo = mid;
        else hi = mid;
    }
    const ImgJob j = jobs[lo];
    const int local = (int)(b - j.tile0), tc = j.cols / kImgTile;
    const int r0 = kImgTile * (local / tc), c0 = kImgTile * (local % tc);
    const int t = threadIdx.x, r = t >> 3, q = t & 7;

    const f32x4 v = *reinterpret_cast<const f32x4 *>(j.src + (size_t)(r0 + r) * j.cols + c0 + 4 * q);
    const bf16x4 o = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
    *reinterpret_cast<bf16x4 *>(j.img + (size_t)(r0 + r) * j.cols + c0 + 4 * q) = o;
    if (!j.img_t) return;      // the same for the whole workgroup
#pragma unroll
    for (int e = 0; e < 4; ++e) tile[r * kImgLd + 4 * q + e] = o[e];
    __syncthreads();
    bf16x4 u;                  // row c0 + r of the transposed image, its elements r0 + 4 q .. r0 + 4 q + 3
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = tile[(4 * q + e) * kImgLd + r];
    *reinterpret_cast<bf16x4 *>(j.img_t + (size_t)(c0 + r) * j.rows + r0 + 4 * q) = u;
}

}  // namespace

}  // namespace rqhip

using namespace rqhip;

extern "C" size_t rqhip_bf16_images_job_bytes(int n_jobs) { return n_jobs > 0 ? (size_t)n_jobs * sizeof(ImgJob) : 0; }

extern "C" int rqhip_bf16_images_fill_jobs(void *host_jobs, const float *const *src, rqhip_bf16_t *const *img,
                                           rqhip_bf16_t *const *img_t, const int64_t *rows, const int64_t *cols, int n_jobs,
                                           int64_t *n_tiles) {
    const char *who = "bf16_images_fill_jobs";
    if (n_jobs < 0) {
        set_error("%s: bad size (n_jobs=%d)", who, n_jobs);
        return RQHIP_EARG;
    }
    if (any_null(n_tiles)) {
        set_error("%s: null pointer (n_tiles)", who);
        return RQHIP_EARG;
    }
    *n_tiles = 0;
    if (n_jobs == 0) return RQHIP_OK;
    if (any_null(host_jobs, src, img, rows, cols)) {
        set_error("%s: null pointer (host_jobs, src, img, rows, cols)", who);
        return RQHIP_EARG;
    }
    if (reinterpret_cast<uintptr_t>(host_jobs) & 7) {
        set_error("%s: host_jobs must be 8-byte aligned", who);
        return RQHIP_EARG;
    }
    ImgJob *jobs = reinterpret_cast<ImgJob *>(host_jobs);
    long long tiles = 0;
    for (int j = 0; j < n_jobs; ++j) {
        rqhip_bf16_t *t = img_t ? img_t[j] : nullptr;
        if (!src[j] || !img[j]) {
            set_error("%s: null pointer (src[%d] or img[%d])", who, j, j);
            return RQHIP_EARG;
        }
        if (!all_aligned16(src[j], img[j], t)) {
            set_error("%s: src[%d], img[%d] and img_t[%d] must be 16-byte aligned", who, j, j, j);
            return RQHIP_EARG;
        }
        if (rows[j] < kImgTile || cols[j] < kImgTile || rows[j] % kImgTile || cols[j] % kImgTile ||
            rows[j] > (1 << 30) || cols[j] > (1 << 30)) {
            set_error("%s: job %d is %lld x %lld: only positive multiples of %d are implemented", who, j, (long long)rows[j],
                      (long long)cols[j], kImgTile);
            return RQHIP_EUNSUPPORTED;
        }
        jobs[j].src = src[j];
        jobs[j].img = reinterpret_cast<__bf16 *>(img[j]);
        jobs[j].img_t = reinterpret_cast<__bf16 *>(t);
        jobs[j].rows = (int)rows[j], jobs[j].cols = (int)cols[j];
        jobs[j].tile0 = tiles;
        tiles += (rows[j] / kImgTile) * (cols[j] / kImgTile);
        if (tiles > (1ll << 31) - 1) {
            set_error("%s: more than 2^31 - 1 tiles of %d x %d", who, kImgTile, kImgTile);
            return RQHIP_EUNSUPPORTED;
        }
    }
    *n_tiles = tiles;
    return RQHIP_OK;
}

extern "C" int rqhip_bf16_images(const void *jobs, int n_jobs, int64_t n_tiles, rqhip_stream_t stream) {
    const char *who = "bf16_images";
    if (n_jobs < 0) {
        set_error("%s: bad size (n_jobs=%d)", who, n_jobs);
        return RQHIP_EARG;
    }
    if (n_jobs == 0) return RQHIP_OK;
    if (any_null(jobs)) {
        set_error("%s: null pointer (jobs)", who);
        return RQHIP_EARG;
    }
    if (!aligned16(jobs)) {
        set_error("%s: the job table must be 16-byte aligned", who);
        return RQHIP_EARG;
    }
    if (n_tiles < n_jobs || n_tiles > (1ll << 31) - 1) {
        set_error("%s: n_tiles=%lld is not the tile count of %d jobs (rqhip_bf16_images_fill_jobs returns it)", who,
                  (long long)n_tiles, n_jobs);
        return RQHIP_EARG;
    }
    hipLaunchKernelGGL(t5_bf16_images_kernel, dim3((unsigned)n_tiles), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const ImgJob *>(jobs), n_jobs);
    RQ_CHECK_LAUNCH("t5_bf16_images_kernel");
    return RQHIP_OK;
}

// rows_pack.hip -- between the padded [B, T, d] layout and the packed [N, d] layout of variable-length rows (gfx950).
//
// rows_pack copies the first cu[b + 1] - cu[b] tokens of every batch row b to rows cu[b] .. of the packed tensor;
// rows_unpack is the inverse and zero-fills the padded tail of every row in the same launch.  Each is the other's
// backward (rqhip/autograd.py).  One thread per 16-byte piece of the PADDED tensor, pieces numbered in its memory
// order: the padded side is one contiguous stream and the packed side contiguous per row.  The table is read through
// packed_group (t5_common.h): a bad entry makes an empty or a short row, never an address.  No LDS, no atomics.
#include "rqhip_common.h"
#include "t5_common.h"

namespace rqhip {

namespace {

constexpr int kRpThreads = 256;

struct RpPlan {
    const float *src;
    float *dst;
    const int *cu;
    long long B, N;
    int T, d4;  // d / 4
};

template <bool PACK>
__global__ __launch_bounds__(kRpThreads) void rows_pack_kernel(RpPlan p) {
    const long long idx = (long long)blockIdx.x * kRpThreads + threadIdx.x;
    const long long per_row = (long long)p.T * p.d4;
    if (idx >= p.B * per_row) return;
    const long long b = idx / per_row;
    const int rem = (int)(idx - b * per_row), t = rem / p.d4, c = rem - t * p.d4;
    long long lo;
    int len;
    packed_group(p.cu, b, p.N, p.T, lo, len);
    const size_t packed = (size_t)(lo + t) * (size_t)p.d4 + (size_t)c;  // read or written only when t < len
    if (PACK) {
        if (t < len)
            reinterpret_cast<float4 *>(p.dst)[packed] = reinterpret_cast<const float4 *>(p.src)[idx];
    } else {
        reinterpret_cast<float4 *>(p.dst)[idx] =
            t < len ? reinterpret_cast<const float4 *>(p.src)[packed] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

int rows_call(const char *who, bool pack, const float *src, const int32_t *cu, int64_t B, int T, int d, int64_t N,
              float *dst, rqhip_stream_t stream) {
    if (B < 0 || T < 1 || d < 4 || d % 4 != 0 || (int64_t)T * (d / 4) >= (1ll << 31) || N < 0 || N > B * (int64_t)T ||
        N >= (1ll << 31)) {
        set_error("%s: bad sizes (B=%lld, T=%d, d=%d, N=%lld): d a multiple of 4, 0 <= N <= B * T, N < 2^31", who,
                  (long long)B, T, d, (long long)N);
        return RQHIP_EARG;
    }
    if (B == 0) return RQHIP_OK;
    if (!cu || (N > 0 && any_null(pack ? dst : src)) || any_null(pack ? src : dst)) {
        set_error("%s: null pointer (src, cu, dst)", who);
        return RQHIP_EARG;
    }
    if (!all_aligned16(src, dst)) {
        set_error("%s: src and dst must be 16-byte aligned", who);
        return RQHIP_EARG;
    }
    const long long n = (long long)B * T * (d / 4);
    if (n >= (1ll << 31) * kRpThreads) {
        set_error("%s: B=%lld rows of %d tokens of %d floats exceed the launch's index range", who, (long long)B, T, d);
        return RQHIP_EUNSUPPORTED;
    }
    RpPlan p;
    p.src = src, p.dst = dst, p.cu = cu, p.B = B, p.N = N, p.T = T, p.d4 = d / 4;
    const dim3 grid((unsigned)((n + kRpThreads - 1) / kRpThreads)), wg(kRpThreads);
    if (pack)
        hipLaunchKernelGGL(rows_pack_kernel<true>, grid, wg, 0, reinterpret_cast<hipStream_t>(stream), p);
    else
        hipLaunchKernelGGL(rows_pack_kernel<false>, grid, wg, 0, reinterpret_cast<hipStream_t>(stream), p);
    RQ_CHECK_LAUNCH("rows_pack_kernel");
    return RQHIP_OK;
}

}  // namespace

}  // namespace rqhip

using namespace rqhip;

extern "C" int rqhip_rows_pack_supported(int d) { return d >= 4 && d % 4 == 0; }

extern "C" int rqhip_rows_pack(const float *x, const int32_t *cu, int64_t B, int T, int d, int64_t N, float *out,
                               rqhip_stream_t stream) {
    return rows_call("rows_pack", true, x, cu, B, T, d, N, out, stream);
}

extern "C" int rqhip_rows_unpack(const float *x, const int32_t *cu, int64_t B, int T, int d, int64_t N, float *out,
                                 rqhip_stream_t stream) {
    return rows_call("rows_unpack", false, x, cu, B, T, d, N, out, stream);
}

// seq_batch.hip -- the retrieval model's training batch in one launch (gfx950): user histories held on the device in CSR
// form, the tokenizer's cached id table and two random integers per row -> a whole TokenizedSeqBatch (semantics in
// include/rqhip.h; data/processed.py:seq_window is the window law this file restates).
//
// A batch row has S + 1 item slots: the S history positions and the target.  An item slot is w int64s, cut into pieces
// of V ids (V = 2, one 16-byte access, when w is even and every id tensor is 16-byte aligned; else V = 1).  One thread
// per piece, pieces numbered in the order of sem_ids' memory: consecutive lanes store consecutive addresses, and the
// lanes of one slot read one table row.  Every thread recomputes its row's window from offsets and the draws (two loads
// and a few integer operations, the same for all lanes of a row).  No LDS, no atomics, no workspace.
#include "rqhip_common.h"
#include "t5_common.h"

namespace rqhip {

namespace {

constexpr int kSbMinW = 2, kSbMaxW = 9;
constexpr int kSbMinS = 2, kSbMaxS = 256;
constexpr int kSbThreads = 256;

typedef long long i64x2 __attribute__((ext_vector_type(2)));

bool sb_supported(int w, int S) { return w >= kSbMinW && w <= kSbMaxW && S >= kSbMinS && S <= kSbMaxS; }

struct SbPlan {
    const long long *offsets, *items, *fut, *user, *rows, *draws, *table;
    long long U, nnz, B, n_items;
    int w, S;
    long long *sem_ids, *sem_ids_fut, *user_ids, *token_type, *token_type_fut;
    unsigned char *seq_mask;
};

template <int V>
struct SbPiece;
template <>
struct SbPiece<1> {
    typedef long long ids;
    typedef unsigned char mask;
    static __device__ __forceinline__ ids fill(long long v) { return v; }
    static __device__ __forceinline__ ids count(int c) { return c; }
};
template <>
struct SbPiece<2> {
    typedef i64x2 ids;
    typedef unsigned short mask;
    static __device__ __forceinline__ ids fill(long long v) { return ids{v, v}; }
    static __device__ __forceinline__ ids count(int c) { return ids{c, c + 1}; }
};

// The window of row r (data/processed.py:seq_window): first history index, history count and the target's index in the
// user's sequence seq = items[lo .. lo + n_hist) followed by fut[r]; fut_pos == n_hist names fut[r].
__device__ __forceinline__ void sb_window(const SbPlan &p, long long b, long long n_hist, long long &first,
                                          long long &count, long long &fut_pos) {
    if (!p.draws) {
        count = n_hist < p.S ? n_hist : p.S;
        first = n_hist - count;
        fut_pos = n_hist;
        return;
    }
    const long long n = n_hist + 1;
    const unsigned long long u0 = (unsigned long long)p.draws[2 * b], u1 = (unsigned long long)p.draws[2 * b + 1];
    const long long start = (long long)(u0 % (unsigned long long)((n > 3 ? n - 3 : 0) + 1));
    long long end = start + 3 + (long long)(u1 % (unsigned long long)(p.S - 1));
    end = end < n ? end : n;
    first = start, count = end - start - 1, fut_pos = end - 1;   // start < n, so end - start >= 1
}

template <int V>
__global__ __launch_bounds__(kSbThreads) void seq_batch_kernel(SbPlan p) {
    typedef typename SbPiece<V>::ids ids_t;
    typedef typename SbPiece<V>::mask mask_t;
    const int pieces = p.w / V;
    const long long t = (long long)blockIdx.x * kSbThreads + threadIdx.x;
    if (t >= p.B * (p.S + 1) * pieces) return;
    const int c = (int)(t % pieces) * V;                  // first column of this piece inside its item
    const long long slot = t / pieces, b = slot / (p.S + 1);
    const int i = (int)(slot % (p.S + 1));                // history position, or S: the target

    // this row's user and the bounds of its history; a user index outside [0, U) or offsets outside [0, nnz] make an
    // empty row, never an address
    const long long r = p.rows[b];
    const bool known = r >= 0 && r < p.U;
    long long lo = 0, hi = 0;
    if (known) {
        lo = p.offsets[r], hi = p.offsets[r + 1];
        lo = lo < 0 ? 0 : (lo > p.nnz ? p.nnz : lo);
        hi = hi < lo ? lo : (hi > p.nnz ? p.nnz : hi);
    }
    const long long n_hist = hi - lo;
    long long first, count, fut_pos;
    sb_window(p, b, n_hist, first, count, fut_pos);

    long long item = -1;
    if (known) {
        if (i < p.S) {
            if (i < count) item = p.items[lo + first + i];            // first + i <= fut_pos - 1 < n_hist
        } else {
            item = fut_pos < n_hist ? p.items[lo + fut_pos] : p.fut[r];
        }
    }
    const bool valid = item >= 0 && item < p.n_items;     // anything else is padding: nothing is read outside the table
    ids_t v = SbPiece<V>::fill(-1);
    if (valid) v = *reinterpret_cast<const ids_t *>(p.table + item * p.w + c);

    if (i < p.S) {
        const long long e = (b * p.S + i) * p.w + c;
        *reinterpret_cast<ids_t *>(p.sem_ids + e) = v;
        *reinterpret_cast<mask_t *>(p.seq_mask + e) = valid ? (mask_t)(V == 2 ? 0x0101 : 0x01) : (mask_t)0;
        if (p.token_type) *reinterpret_cast<ids_t *>(p.token_type + e) = SbPiece<V>::count(c);
    } else {
        const long long e = b * p.w + c;
        *reinterpret_cast<ids_t *>(p.sem_ids_fut + e) = v;
        if (p.token_type_fut) *reinterpret_cast<ids_t *>(p.token_type_fut + e) = SbPiece<V>::count(c);
        if (c == 0) p.user_ids[b] = known ? p.user[r] : -1;
    }
}

}  // namespace

}  // namespace rqhip

using namespace rqhip;

extern "C" int rqhip_seq_batch_supported(int w, int S) { return sb_supported(w, S); }

extern "C" int rqhip_seq_batch(const int64_t *offsets, const int64_t *items, const int64_t *fut, const int64_t *user,
                               int64_t U, int64_t nnz, const int64_t *rows, int64_t B, const int64_t *draws,
                               const int64_t *table, int64_t n_items, int w, int S, int64_t *sem_ids, uint8_t *seq_mask,
                               int64_t *sem_ids_fut, int64_t *user_ids, int64_t *token_type, int64_t *token_type_fut,
                               rqhip_stream_t stream) {
    if (B < 0 || U < 0 || nnz < 0 || n_items < 0) {
        set_error("seq_batch: bad sizes (B=%lld, U=%lld, nnz=%lld, n_items=%lld)", (long long)B, (long long)U,
                  (long long)nnz, (long long)n_items);
        return RQHIP_EARG;
    }
    if (!sb_supported(w, S)) {
        set_error("seq_batch: w=%d, S=%d: only w in %d .. %d and S in %d .. %d are implemented", w, S, kSbMinW, kSbMaxW,
                  kSbMinS, kSbMaxS);
        return RQHIP_EARG;
    }
    if (B == 0) return RQHIP_OK;
    if (any_null(offsets, fut, user, rows, sem_ids, seq_mask, sem_ids_fut, user_ids) || (nnz > 0 && !items) ||
        (n_items > 0 && !table)) {
        set_error("seq_batch: null pointer (offsets, items, fut, user, rows, table, sem_ids, seq_mask, sem_ids_fut, user_ids)");
        return RQHIP_EARG;
    }
    const long long threads = (long long)B * (S + 1) * w;    // the one-id form: the most threads either form starts
    if (threads >= (1ll << 31)) {
        set_error("seq_batch: B=%lld rows of %d item slots of %d ids exceed the launch's index range", (long long)B, S + 1, w);
        return RQHIP_EUNSUPPORTED;
    }
    SbPlan p;
    p.offsets = reinterpret_cast<const long long *>(offsets), p.items = reinterpret_cast<const long long *>(items);
    p.fut = reinterpret_cast<const long long *>(fut), p.user = reinterpret_cast<const long long *>(user);
    p.rows = reinterpret_cast<const long long *>(rows), p.draws = reinterpret_cast<const long long *>(draws);
    p.table = reinterpret_cast<const long long *>(table);
    p.U = U, p.nnz = nnz, p.B = B, p.n_items = n_items, p.w = w, p.S = S;
    p.sem_ids = reinterpret_cast<long long *>(sem_ids), p.sem_ids_fut = reinterpret_cast<long long *>(sem_ids_fut);
    p.user_ids = reinterpret_cast<long long *>(user_ids), p.token_type = reinterpret_cast<long long *>(token_type);
    p.token_type_fut = reinterpret_cast<long long *>(token_type_fut), p.seq_mask = seq_mask;
    // w even: an item's row is a whole number of 16-byte pieces in the table and in every output (and of byte pairs in
    // the mask); buffers that are not aligned for them take the one-id form
    const bool wide = w % 2 == 0 && all_aligned16(table, sem_ids, sem_ids_fut, token_type, token_type_fut) &&
                      (reinterpret_cast<uintptr_t>(seq_mask) & 1) == 0;
    const long long n = threads / (wide ? 2 : 1);
    const dim3 grid((unsigned)((n + kSbThreads - 1) / kSbThreads)), wg(kSbThreads);
    if (wide)
        hipLaunchKernelGGL(seq_batch_kernel<2>, grid, wg, 0, reinterpret_cast<hipStream_t>(stream), p);
    else
        hipLaunchKernelGGL(seq_batch_kernel<1>, grid, wg, 0, reinterpret_cast<hipStream_t>(stream), p);
    RQ_CHECK_LAUNCH("seq_batch_kernel");
    return RQHIP_OK;
}

// sid_items.hip -- from generated semantic-id tuples to corpus item numbers (gfx950).
//
//   item index : exact map (L-tuple, dedup rank) -> item number, the inverse of SemanticIdTokenizer._lookup
//                (modules/tokenizer/semids.py).  Several items share a tuple; the tokenizer tells them apart by the dedup
//                column "how many earlier items have this tuple", which the decoder never generates.
//   lookup     : one (tuple, rank) query per thread -> item number or -1.
//   top-n      : per user, the beams of `generate` (best first) expanded to the items that carry their tuples, in
//                ascending dedup rank == ascending item number, without the items of the user's history, cut at n.
//
// Design, as csrc/sid_match.hip.  The corpus is fixed, so the map is built ONCE: one open-addressing table (load factor
// <= 1/2) whose slots hold row numbers, next to an int32 copy of the dedup ranks.  Rows are unique in (tuple, rank), so
// an insertion never meets "already present" and compares nothing.  Membership is decided by comparing the stored row's
// ids and rank with the query, never by the hash alone: slot positions depend on the insertion race, answers do not.
//
// Index layout (opaque to callers): slots_for(N) int32 slots, then N int32 ranks.  A rank outside [0, 2^31) cannot be a
// dedup rank of a corpus below 2^30 rows; such a row is stored with rank -1 and no query finds it.
//
// The top-n kernel runs one wave per user with lane b owning beam b (hence k <= 64), four users per 256-thread
// workgroup.  A lane walks its tuple's group r = 0, 1, 2, ... twice: once to count the items it can give (capped at n),
// and, after a wave-wide exclusive scan of the counts has given it its output offset, once to write them.  Each probe of
// a walk either emits an item, hits a distinct history item of the user, or ends the group, so a walk makes at most
// n + (distinct history items) + 1 probes.  The wave writes the -1 / -inf tail of its own row: no fill launch, no
// atomics, the same bits on every run and on every build of the index.
#include <limits.h>
#include <math.h>

#include "rqhip_common.h"
#include "sid_hash.h"

namespace rqhip {

constexpr int kItemsUsersPerBlock = 4;  // waves per workgroup of items_topn_kernel, one user each

struct ItemIndex {
    const int *table;  // [mask + 1] row numbers, -1 = empty
    const int *rank;   // [N]
    unsigned mask;
    const int64_t *corpus;
    long long ld;
    int L;
};

// the row with tuple t[0:L] and dedup rank r, or -1
__device__ __forceinline__ int item_find(const ItemIndex &ix, const int64_t *__restrict__ t, int64_t r) {
    if (r < 0 || r > (int64_t)INT_MAX) return -1;
    unsigned hsh = kSidHashSeed;
    for (int c = 0; c < ix.L; ++c) hsh = sid_hash_step(hsh, t[c]);
    hsh = sid_hash_step(hsh, r);
    unsigned s = sid_hash_final(hsh) & ix.mask;
    for (;;) {  // ends: the table has at least as many empty slots as rows
        const int prev = ix.table[s];
        if (prev == -1) return -1;
        bool same = ix.rank[prev] == (int)r;
        const int64_t *other = ix.corpus + (size_t)prev * ix.ld;
        for (int c = 0; c < ix.L && same; ++c) same = other[c] == t[c];
        if (same) return prev;
        s = (s + 1) & ix.mask;
    }
}

// one thread per corpus row: keeps its rank as int32 and inserts itself
__global__ __launch_bounds__(256) void item_build_kernel(const int64_t *__restrict__ corpus, long long N, int L,
                                                         long long ld, const int64_t *__restrict__ rank,
                                                         int *__restrict__ table, int *__restrict__ rank32,
                                                         unsigned mask) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int64_t r = rank[i];
    const bool ok = r >= 0 && r <= (int64_t)INT_MAX;
    rank32[i] = ok ? (int)r : -1;
    if (!ok) return;  // no query can name this row
    const int64_t *mine = corpus + (size_t)i * ld;
    unsigned hsh = kSidHashSeed;
    for (int c = 0; c < L; ++c) hsh = sid_hash_step(hsh, mine[c]);
    hsh = sid_hash_step(hsh, r);
    unsigned s = sid_hash_final(hsh) & mask;
    while (atomicCAS(&table[s], -1, (int)i) != -1) s = (s + 1) & mask;
}

// one thread per query (tuple, rank)
__global__ __launch_bounds__(256) void item_lookup_kernel(ItemIndex ix, const int64_t *__restrict__ ids, long long P,
                                                          long long ld_ids, int64_t *__restrict__ items) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= P) return;
    const int64_t *mine = ids + (size_t)q * ld_ids;
    items[q] = (int64_t)item_find(ix, mine, mine[ix.L]);
}

// The history items of one user that carry one lane's tuple: found once per lane, so that a probe of the walk compares
// ranks only.  The first 64 items are a bit mask; `rest` says that an item beyond them has the tuple too, and those are
// then compared in full.  h == nullptr: nothing to exclude.
struct SeenItems {
    const int64_t *h;
    unsigned long long mask;
    bool rest;
};

// whether history item j at h has tuple t (an item with any negative id, its rank included, is padding)
__device__ __forceinline__ bool history_has_tuple(const int64_t *__restrict__ h, long long j, int L,
                                                  const int64_t *__restrict__ t) {
    const int64_t *it = h + (size_t)j * (L + 1);
    bool same = it[L] >= 0;
    for (int c = 0; c < L; ++c) same &= (it[c] == t[c]) & (it[c] >= 0);  // no early exit: the loads do not wait for each other
    return same;
}

__device__ __forceinline__ SeenItems seen_items(const int64_t *__restrict__ h, long long T, int L,
                                                const int64_t *__restrict__ t) {
    SeenItems s{nullptr, 0ull, false};
    const int head = (int)(T < 64 ? T : 64);
#pragma unroll 4
    for (int j = 0; j < head; ++j)
        if (history_has_tuple(h, j, L, t)) s.mask |= 1ull << j;
    for (long long j = 64; j < T; ++j) s.rest |= history_has_tuple(h, j, L, t);
    if (s.mask || s.rest) s.h = h;
    return s;
}

// whether (the lane's tuple t, rank r >= 0) is one of the user's history items
__device__ __forceinline__ bool in_history(const SeenItems &s, long long T, int L, const int64_t *__restrict__ t,
                                           int64_t r) {
    bool found = false;
    for (unsigned long long m = s.mask; m; m &= m - 1) {
        const int j = __builtin_ctzll(m);
        found |= s.h[(size_t)j * (L + 1) + L] == r;
    }
    if (s.rest)
        for (long long j = 64; j < T; ++j) found |= history_has_tuple(s.h, j, L, t) && s.h[(size_t)j * (L + 1) + L] == r;
    return found;
}

// One walk over the group of tuple t: the items of ranks 0, 1, ... that are not in the history, at most `want` of them;
// written to out[0 .. ) when out is not null.  Returns how many.
__device__ __forceinline__ int walk_group(const ItemIndex &ix, const int64_t *__restrict__ t, const SeenItems &seen,
                                          long long T, int want, int64_t *__restrict__ out) {
    int got = 0;
    for (int64_t r = 0; got < want; ++r) {
        const int item = item_find(ix, t, r);
        if (item < 0) break;
        if (seen.h && in_history(seen, T, ix.L, t, r)) continue;
        if (out) out[got] = (int64_t)item;
        ++got;
    }
    return got;
}

__global__ __launch_bounds__(64 * kItemsUsersPerBlock) void items_topn_kernel(
    ItemIndex ix, const int64_t *__restrict__ beams, const float *__restrict__ scores, long long B, int k,
    const int64_t *__restrict__ history, long long T, long long ld_hist, int n, int64_t *__restrict__ items,
    float *__restrict__ item_scores) {
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * kItemsUsersPerBlock + (threadIdx.x >> 6);
    if (u >= B) return;  // the whole wave leaves
    const int L = ix.L;
    const int64_t *ubeams = beams + (size_t)u * k * L;
    const float *uscores = scores + (size_t)u * k;
    const int64_t *mine = ubeams + (size_t)lane * L;

    float score = -INFINITY;
    bool live = false;
    if (lane < k) {
        score = uscores[lane];
        live = score > -INFINITY;  // false for -inf and for NaN
        // the same tuple in an earlier contributing beam: that beam gives the group's items (no early exit: the loads
        // of the earlier beams do not wait for each other)
        bool repeated = false;
        for (int b = 0; b < lane; ++b) {
            const int64_t *other = ubeams + (size_t)b * L;
            bool same = uscores[b] > -INFINITY;
            for (int c = 0; c < L; ++c) same &= other[c] == mine[c];
            repeated |= same;
        }
        live = live && !repeated;
    }

    // the user's history items that have this lane's tuple
    SeenItems hist{nullptr, 0ull, false};
    if (live && history && T > 0) hist = seen_items(history + (size_t)u * ld_hist, T, L, mine);

    const int count = live ? walk_group(ix, mine, hist, T, n, nullptr) : 0;  // <= n <= 256

    // wave-wide inclusive scan of the counts (<= 64 * 256, no overflow)
    int incl = count;
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    const int offset = incl - count;
    const int total = min(__shfl(incl, 63, 64), n);

    int64_t *uitems = items + (size_t)u * n;
    float *uitem_scores = item_scores + (size_t)u * n;
    const int take = min(count, n - min(offset, n));
    if (take > 0) {
        walk_group(ix, mine, hist, T, take, uitems + offset);
        for (int j = 0; j < take; ++j) uitem_scores[offset + j] = score;
    }
    for (int j = total + lane; j < n; j += 64) {
        uitems[j] = -1;
        uitem_scores[j] = -INFINITY;
    }
}

}  // namespace rqhip

using namespace rqhip;

extern "C" size_t rqhip_sid_item_index_bytes(int64_t N) {
    if (N < 0) return 0;
    return ((size_t)slots_for(N) + (size_t)N) * sizeof(int);
}

static int check_item_corpus(const char *who, const int64_t *corpus, int64_t N, int L, int64_t ld) {
    if (N < 0 || L < 1 || ld < L || (N > 0 && !corpus)) {
        set_error("%s: bad corpus (N=%lld, L=%d, ld=%lld, corpus %s; N >= 0, L >= 1, ld >= L)", who, (long long)N, L,
                  (long long)ld, corpus ? "given" : "null");
        return RQHIP_EARG;
    }
    if (L + 1 > RQHIP_MAX_PREFIX_LEN) {
        set_error("%s: L=%d ids and the dedup rank exceed RQHIP_MAX_PREFIX_LEN=%d (L + 1 <= %d)", who, L,
                  RQHIP_MAX_PREFIX_LEN, RQHIP_MAX_PREFIX_LEN);
        return RQHIP_EUNSUPPORTED;
    }
    if (N >= (1ll << 30)) {
        set_error("%s: N=%lld exceeds the 2^30 rows this implementation indexes with 32 bits", who, (long long)N);
        return RQHIP_EUNSUPPORTED;
    }
    return RQHIP_OK;
}

static int check_item_index(const char *who, const void *index, size_t index_bytes, int64_t N) {
    const size_t need = rqhip_sid_item_index_bytes(N);
    if (!index || index_bytes < need) {
        set_error("%s: index buffer too small for N=%lld (%zu < %zu)", who, (long long)N, index ? index_bytes : (size_t)0,
                  need);
        return RQHIP_EWORKSPACE;
    }
    return RQHIP_OK;
}

static ItemIndex item_index(const void *index, const int64_t *corpus, int64_t N, int L, int64_t ld) {
    const unsigned long long slots = slots_for(N);
    const int *table = reinterpret_cast<const int *>(index);
    return ItemIndex{table, table + slots, (unsigned)(slots - 1), corpus, (long long)ld, L};
}

extern "C" int rqhip_sid_item_index_build(const int64_t *corpus, int64_t N, int L, int64_t ld, const int64_t *rank,
                                          void *index, size_t index_bytes, rqhip_stream_t stream) {
    if (int rc = check_item_corpus("sid_item_index_build", corpus, N, L, ld)) return rc;
    if (N > 0 && !rank) {
        set_error("sid_item_index_build: null rank (the dedup column, [N] int64)");
        return RQHIP_EARG;
    }
    if (int rc = check_item_index("sid_item_index_build", index, index_bytes, N)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned long long slots = slots_for(N);
    if (int rc = fill_words(index, 0xffffffffu, (size_t)slots * sizeof(int), s)) return rc;
    if (N == 0) return RQHIP_OK;
    const int tb = 256;
    int *table = reinterpret_cast<int *>(index);
    hipLaunchKernelGGL(item_build_kernel, dim3((unsigned)((N + tb - 1) / tb)), dim3(tb), 0, s, corpus, (long long)N, L,
                       (long long)ld, rank, table, table + slots, (unsigned)(slots - 1));
    RQ_CHECK_LAUNCH("item_build_kernel");
    return RQHIP_OK;
}

extern "C" int rqhip_sid_item_lookup(const void *index, size_t index_bytes, const int64_t *corpus, int64_t N, int L,
                                     int64_t ld, const int64_t *ids, int64_t P, int64_t ld_ids, int64_t *items,
                                     rqhip_stream_t stream) {
    if (int rc = check_item_corpus("sid_item_lookup", corpus, N, L, ld)) return rc;
    if (P < 0 || ld_ids < L + 1 || (P > 0 && (!ids || !items))) {
        set_error("sid_item_lookup: bad query (P=%lld, ld_ids=%lld; P >= 0, ld_ids >= L + 1 = %d, ids and items given)",
                  (long long)P, (long long)ld_ids, L + 1);
        return RQHIP_EARG;
    }
    if (P >= (1ll << 39)) {
        set_error("sid_item_lookup: P=%lld is too large (P < 2^39)", (long long)P);
        return RQHIP_EUNSUPPORTED;
    }
    if (int rc = check_item_index("sid_item_lookup", index, index_bytes, N)) return rc;
    if (P == 0) return RQHIP_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int tb = 256;
    hipLaunchKernelGGL(item_lookup_kernel, dim3((unsigned)((P + tb - 1) / tb)), dim3(tb), 0, s,
                       item_index(index, corpus, N, L, ld), ids, (long long)P, (long long)ld_ids, items);
    RQ_CHECK_LAUNCH("item_lookup_kernel");
    return RQHIP_OK;
}

extern "C" int rqhip_sid_items_topn(const void *index, size_t index_bytes, const int64_t *corpus, int64_t N, int L,
                                    int64_t ld, const int64_t *beams, const float *scores, int64_t B, int k,
                                    const int64_t *history, int64_t T, int64_t ld_hist, int n, int64_t *items,
                                    float *item_scores, rqhip_stream_t stream) {
    if (int rc = check_item_corpus("sid_items_topn", corpus, N, L, ld)) return rc;
    if (k < 1 || k > 64) {
        set_error("sid_items_topn: k=%d beams per user (1 <= k <= 64: one lane per beam)", k);
        return k < 1 ? RQHIP_EARG : RQHIP_EUNSUPPORTED;
    }
    if (n < 1 || n > 256) {
        set_error("sid_items_topn: n=%d items per user (1 <= n <= 256)", n);
        return n < 1 ? RQHIP_EARG : RQHIP_EUNSUPPORTED;
    }
    if (B < 0 || T < 0 || (B > 0 && (!beams || !scores || !items || !item_scores))) {
        set_error("sid_items_topn: bad arguments (B=%lld, T=%lld; B >= 0, T >= 0, beams, scores, items and item_scores "
                  "given)", (long long)B, (long long)T);
        return RQHIP_EARG;
    }
    if (history && (T >= (1ll << 31) || ld_hist < T * (L + 1))) {
        set_error("sid_items_topn: bad history (T=%lld, ld_hist=%lld; T < 2^31, ld_hist >= T * (L + 1) = %lld)",
                  (long long)T, (long long)ld_hist, (long long)T * (L + 1));
        return RQHIP_EARG;
    }
    if (B >= (1ll << 31)) {
        set_error("sid_items_topn: B=%lld is too large (B < 2^31)", (long long)B);
        return RQHIP_EUNSUPPORTED;
    }
    if (int rc = check_item_index("sid_items_topn", index, index_bytes, N)) return rc;
    if (B == 0) return RQHIP_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned gb = (unsigned)((B + kItemsUsersPerBlock - 1) / kItemsUsersPerBlock);
    hipLaunchKernelGGL(items_topn_kernel, dim3(gb), dim3(64 * kItemsUsersPerBlock), 0, s,
                       item_index(index, corpus, N, L, ld), beams, scores, (long long)B, k, history, (long long)T,
                       (long long)ld_hist, n, items, item_scores);
    RQ_CHECK_LAUNCH("items_topn_kernel");
    return RQHIP_OK;
}

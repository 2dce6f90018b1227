// What the two halves of the mapping driver share: mm_map.hip (sketch -> seeds -> anchors ->
// sort, the long join's anchor set, regions, records) and mm_chainset.hip (groups -> DP ->
// backtrack -> chain list over one anchor set).
#pragma once
#include "mm_common.hpp"
#include "sort.hpp"

namespace hymet {
namespace mm {

#define LAUNCH1(kern, n, ...)                                                                           \
    do {                                                                                                \
        if ((n) > 0) {                                                                                  \
            hipLaunchKernelGGL(kern, dim3((unsigned)cdiv((n), 256)), dim3(256), 0, ctx->stream, __VA_ARGS__); \
            HY_CHECK_LAUNCH(#kern);                                                                     \
        }                                                                                               \
    } while (0)

namespace {

__device__ __forceinline__ int upper_idx(const int64_t *off, int n, int64_t v) {  // last s with off[s] <= v
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void iota_u32_kernel(uint32_t *a, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = (uint32_t)i;
}

template <typename T>
__global__ void gather_kernel(const T *__restrict__ src, const uint32_t *__restrict__ idx, T *__restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

}  // namespace

// the library's stable LSD radix sort (sort.hpp), profiled under `tag`; keys / vals point at
// the sorted data on return
template <typename K, typename V, int RB = 0>
static int sort_pairs(hymet_ctx *ctx, K *&keys, K *&keys_alt, V *&vals, V *&vals_alt, int64_t n, int begin_bit, int end_bit,
                      const char *tag = "radix_sort") {
    if (n <= 1) return HYMET_OK;
    ProfScope _ps(ctx, tag, 2.0 * (double)n * (sizeof(K) + sizeof(V)) * (double)((end_bit - begin_bit + 7) / 8));
    return radix_sort_pairs(ctx, keys, keys_alt, vals, vals_alt, n, begin_bit, end_bit);
}

inline int scan_flags(hymet_ctx *ctx, const uint32_t *flag, int64_t n, DevBuf &pos, int64_t *total) {
    HY_HIP(pos.alloc(8 * (size_t)(n + 1), ctx->stream));
    return exclusive_scan_u32_i64(ctx, flag, pos.as<int64_t>(), n, total);
}

// The most anchors a set may hold: the DP's links p and the backtrack's chain ids are 32-bit
// indices into their set (n < INT32_MAX).  HYMET_ANCHOR_CAP lowers it, so a test reaches the
// error with a small input.
inline int64_t anchor_cap() { return env_int("HYMET_ANCHOR_CAP", INT32_MAX - 1, 1, INT32_MAX - 1); }

// An anchor set sorted by (query, x, y): arrays + per-query offsets (device + host).  y is
// span << 32 | query position, and the span is one value for the whole set (k, for every
// minimizer of a non-HPC sketch): the array holds the low word alone.
struct AnchorSet {
    DevBuf ax;            // 8 B per anchor: rev << 63 | rid << 32 | target position
    DevBuf ay;            // 4 B per anchor: y's low word
    int span = 0;         // y's high word
    int64_t n = 0;
    DevBuf d_off;
    DevBuf hb;            // group-head bitmap (head_bits_bytes(n)): bit i where x >> 32 changes
    bool has_hb = false;  // hb written by whoever built the set; else chain_set derives it from x
    DevBuf ax32;          // x's low words (the chaining kernels read 4 B of x per anchor, not 8)
    bool has_x32 = false;
};

// Chains of an anchor set: compacted anchors (chain by chain, chains ordered by first
// anchor) + chain scores/counts + per-query chain offsets.
struct ChainSet {
    DevBuf cu, cboff;          // per chain: score<<32 | count; offset of its anchors in chain order
    DevBuf ids, cfirst;        // backtrack output (each chain end -> start) and each chain's first slot
    const uint64_t *ax = nullptr;  // the chained anchor set (alive as long as the chains)
    const uint32_t *ay = nullptr;
    const uint32_t *ax32 = nullptr;  // its x low words (chain_set derives them where the set's writer left them out)
    int span = 0;
    DevBuf cq;              // query of each chain
    int64_t n_anchor = 0, n_chain = 0;
    DevBuf d_qc, d_qb;  // n_q + 1 chain / chain-order anchor offsets per query
};

// A first pass followed by the long join (map.c's rmq rescue): chain_set flags the re-chained
// queries from its chain list; their chains take no slots in the chain order (their regions
// are never built) but stay marked in the chained anchor set, which the long join compacts.
struct LeanJoin {
    const int64_t *qlen;
    int rescue_size;
    float rescue_ratio;
    DevBuf flag;                 // per query: re-chained
    DevBuf mark;                 // the backtrack's marks, one byte per anchor of the set (+16 bytes for 16-byte
                                 // loads): 2 = in a kept chain
    DevBuf qb2;                  // n_q + 1 offsets of the re-chained queries' chain anchors
    int64_t n2 = 0;              // their total
};

// chaining + backtrack + compact_a over an anchor set (mm_chainset.hip); with lj, also the
// long join's hand-over
int chain_set(hymet_ctx *ctx, const hymet_mm_opt *opt, float pen_gap, float pen_skip, int bw, AnchorSet &A, int n_q,
              ChainSet &C, LeanJoin *lj = nullptr);
// long join: the flagged queries' marked anchors of S1 (A2 of them, S2.d_off set by the
// caller), compacted in S1's order into S2 with its head bitmap and x low words
int marked_anchor_set(hymet_ctx *ctx, const AnchorSet &S1, const LeanJoin &lj, const uint32_t *flag, int n_q, int64_t A2,
                      AnchorSet &S2);

}  // namespace mm
}  // namespace hymet

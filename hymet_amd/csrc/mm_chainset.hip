// Chains of one sorted anchor set (stages 6-7 of the mapping, mm_map.hip): (query, strand,
// target) groups from the set's head bitmap -> size-descending work list -> the chaining DP
// (mm_chain.hip) -> backtrack order z -> backtrack -> chains ordered by first anchor (compact_a)
// with per-query offsets -> the long join's hand-over (the re-chained queries and their marks).
// chain_set runs these as stages: a stage's temporaries are released when it returns, and what
// a later stage reads travels in the stage's result.  hymet_mm_chain_dp (tests, tools) runs the
// first three on a caller's anchor set.
#include "mm_stages.hpp"

#include <algorithm>
#include <cstdio>

namespace hymet {
namespace mm {

int launch_chain(hymet_ctx *ctx, const int32_t *ax, const uint32_t *ay, int span, const int64_t *g_start, const uint8_t *g_qfirst,
                 const int32_t *order, int32_t n_work, int32_t *f, int32_t *p, int32_t *t_global, int max_dist,
                 int max_dist_inner, int bw, int max_chn_skip, int cap_rmq_size, float pen_gap, float pen_skip,
                 int64_t n_anchors, int64_t n_groups);
int launch_backtrack(hymet_ctx *ctx, const int64_t *g_start, const int32_t *f, const int32_t *p, uint8_t *t,
                     const int32_t *z_cnt, const int32_t *z_idx, int32_t n_groups, const int32_t *order, int32_t n_work,
                     int min_cnt, int min_sc, int max_drop, int32_t *chain_ids, uint64_t *chain_u, int64_t *chain_first,
                     int32_t *n_chains, int64_t n_anchors);

namespace {

// Groups of an anchor set sorted by (query, x, y): a group starts at every non-empty query's
// first anchor and wherever x >> 32 (strand, target) changes.  The x changes come as a bitmap
// from whoever wrote the set -- the grouped sort's writers (AnchorOut::head), the long join's
// compaction, or head_bits_x_kernel for the other paths -- so numbering the groups reads one bit
// per anchor instead of x twice: pass 1 counts the heads per tile of kGTile anchors (64 per
// thread: two bitmap words), a scan of the tile counts, pass 2 writes g_start and each group's
// query-first flag.  A tile's query starts come from the query offsets into an LDS bitmap.
constexpr int kGTile = 16384;

__device__ __forceinline__ uint64_t group_tile_bits(const uint32_t *hb, int64_t n, const int64_t *qoff, int n_q, int64_t t0,
                                                    uint64_t *qs) {
    __shared__ int s_q0;
    const int tid = threadIdx.x;
    const int64_t t1 = min(t0 + kGTile, n);
    const int64_t a0 = t0 + 64 * (int64_t)tid;
    const uint64_t hw = a0 < n ? reinterpret_cast<const uint64_t *>(hb)[a0 >> 6] : 0;
    qs[tid] = 0;
    if (tid == 0) {  // first query whose range ends after t0
        int lo = 0, hi = n_q;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (qoff[mid + 1] <= t0) lo = mid + 1;
            else hi = mid;
        }
        s_q0 = lo;
    }
    __syncthreads();
    for (int q = s_q0 + tid; q < n_q; q += 256) {
        const int64_t a = qoff[q];
        if (a >= t1) break;
        if (a >= t0 && a < qoff[q + 1]) atomicOr((unsigned long long *)&qs[(a - t0) >> 6], 1ull << ((a - t0) & 63));
    }
    __syncthreads();
    const int64_t m = n - a0;  // anchors of this thread's 64 that exist
    const uint64_t live = m >= 64 ? ~0ull : m > 0 ? (1ull << m) - 1 : 0ull;
    return (hw | qs[tid]) & live;
}

__global__ __launch_bounds__(256) void group_heads_count_kernel(const uint32_t *hb, int64_t n, const int64_t *qoff, int n_q,
                                                          uint32_t *tile_cnt) {
    __shared__ uint64_t qs[kGTile / 64];
    __shared__ uint32_t ws[4];
    const uint64_t h = group_tile_bits(hb, n, qoff, n_q, (int64_t)blockIdx.x * kGTile, qs);
    uint32_t c = (uint32_t)__popcll(h);
    for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// g_start of every group, its query-first flag (lchain.c's krmq index-0 quirk) and the
// g_start[G] = n sentinel
__global__ __launch_bounds__(256) void group_heads_write_kernel(const uint32_t *hb, int64_t n, const int64_t *qoff, int n_q,
                                                          const int64_t *tile_off, int64_t *g_start, uint8_t *qfirst,
                                                          int64_t G) {
    __shared__ uint64_t qs[kGTile / 64];
    __shared__ uint32_t ws[4];
    const int64_t t0 = (int64_t)blockIdx.x * kGTile;
    uint64_t h = group_tile_bits(hb, n, qoff, n_q, t0, qs);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t c = (uint32_t)__popcll(h);
    uint32_t inc = c;  // exclusive scan of the threads' counts in anchor order
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) ws[w] = inc;
    __syncthreads();
    int64_t g = tile_off[blockIdx.x] + inc - c;
    for (int k = 0; k < w; k++) g += ws[k];
    const uint64_t qw = qs[threadIdx.x];
    const int64_t a0 = t0 + 64 * (int64_t)threadIdx.x;
    while (h) {
        const int b = __ffsll((unsigned long long)h) - 1;
        h &= h - 1;
        g_start[g] = a0 + b;
        qfirst[g] = (uint8_t)(qw >> b & 1);
        ++g;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) g_start[G] = n;
}

// x's low words of an anchor set written without them (the two-key and test paths)
__global__ void x_low_kernel(const uint64_t *x, int64_t n, uint32_t *x32) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x32[i] = (uint32_t)x[i];
}

// the head bitmap of an anchor set written without one (the two-key and test paths):
// x >> 32 differs from the previous anchor's, a wave's 64 anchors per 64-bit word
__global__ __launch_bounds__(256) void head_bits_x_kernel(const uint64_t *x, int64_t n, uint64_t *hb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool hd = i < n && (i == 0 || (x[i] >> 32) != (x[i - 1] >> 32));
    const uint64_t b = __ballot(hd);
    if ((threadIdx.x & 63) == 0 && i < n) hb[i >> 6] = b;
}

// largest group: the first of the size-descending list, or, when sizes tie at the 16-bit
// key's cap, the largest of that tied prefix
// (out: a mailbox word)
__global__ void max_group_kernel(const int64_t *g_start, const int32_t *order, int32_t G, int64_t *out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t best = 0;
    for (int32_t w = 0; w < G; w++) {
        const int g = order[w];
        const int64_t sz = g_start[g + 1] - g_start[g];
        best = max(best, sz);
        if (sz < 0xffff) break;
    }
    *out = best;
}

// groups of fewer than min_cnt anchors: f = 0, p = -1 (the chaining kernels write f and p of
// the anchors of every work group, so neither needs a pass over the set)
__global__ void nonwork_fp_kernel(const int64_t *g_start, int32_t G, int min_cnt, int32_t *f, int32_t *p) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int64_t a0 = g_start[g], a1 = g_start[g + 1];
    if (a1 - a0 >= min_cnt) return;
    for (int64_t a = a0; a < a1; a++) f[a] = 0, p[a] = -1;
}

// also clears the per-group query-first flags and the z-order list counters
__global__ void group_size_kernel(const int64_t *g_start, int32_t G, int min_cnt, uint32_t *key, uint32_t *gidx,
                                  uint32_t *is_work, uint8_t *qfirst, int32_t *zlists) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < 8) zlists[g] = 0;
    if (g >= G) return;
    if (qfirst) qfirst[g] = 0;
    const int64_t sz = g_start[g + 1] - g_start[g];
    // descending size in 16 bits (two radix passes): groups above 65535 anchors tie at the
    // front, non-work groups (< min_cnt <= 3 anchors) come after every work group
    key[g] = 0xffffu - (uint32_t)min(sz, (int64_t)0xffff);
    gidx[g] = (uint32_t)g;
    is_work[g] = sz >= min_cnt ? 1u : 0u;
}

// ---- backtrack order: z = anchors with f >= min_sc, per group ascending (f, idx) (the
// backtrack walks it from the end: canonical T3).  A group's z entries are kept inside the
// group's own anchor range [g_start[g], g_start[g] + z_cnt[g]), so no global flag scan or
// offset table is needed.  The entries are nearly sorted already: f grows along a colinear
// chain, so a group is a few ascending runs (one per chain or chain piece).
//  * groups of <= kZLane anchors: one lane each, ranks by all-pairs comparison in registers;
//  * larger groups: one wave each reads the group's f once, compacts its z keys (ballot), finds
//    the descents between consecutive keys (the previous key by shuffle) and records the
//    starts of the first kZRuns runs.  A single run is already the order (the wave wrote it).
//    Groups of <= max_runs runs are merged by a flat kernel -- every entry's position is its
//    offset in its own run plus, per other run, a binary search (keys are unique).  Groups
//    with more runs go to a block bitonic sort in LDS (<= kZs entries) or one global radix
//    sort over all such larger groups (lists appended with atomics: the sorted result does
//    not depend on the list order).
constexpr int kZs = 2048;
constexpr int kZRuns = 16;
constexpr int kZmLds = 6144;   // merge groups staged in LDS up to this many entries (48 KB: three blocks per CU)
constexpr int kZmUnit = 2048;  // larger merge groups: units of this many entries, one block each
constexpr int kZLane = 16;
#ifndef HYMET_Z_DEPTH
#define HYMET_Z_DEPTH 8
#endif
constexpr int kZDepth = HYMET_Z_DEPTH;  // f chunks in flight per wave (zorder_wave_kernel)

struct ZParams {
    const int32_t *f;
    const int64_t *g_start;
    const int32_t *order;  // all groups by descending size (the chaining work list, whole)
    int32_t G;
    int min_sc, max_runs;
    int zm_lds, zm_unit;   // kZmLds / kZmUnit (HYMET_ZM_LDS / HYMET_ZM_UNIT in tests)
    uint64_t *zkey;        // n: (f << 32 | idx) at the group's compacted z positions
    int32_t *z_idx;        // n: the order, at the same positions
    int32_t *z_cnt;        // per group: number of z entries
    int32_t *z_runs;       // per group: ascending runs (0 when empty)
    int32_t *run_start;    // per group, kZRuns entries: run starts relative to g_start
    int32_t *lists;        // [0] split, [1] mid count, [2] big count, [3] merge count, [4..5] big total (i64),
                           // [6] merge-unit count
    int32_t *merge_list;   // groups of 2..max_runs runs, for the merge
    int64_t *mergeu_list;  // units (group << 32 | u) of kZmUnit entries of the merge groups above kZmLds
    int32_t *mid_list;     // groups for the block sort
    int32_t *big_list;     // groups for the radix path
    int64_t *big_off;      // their offsets in the radix arrays
    int64_t *mail;         // mailbox words: big count, big total (published by zmerge_kernel)
};

// first list position whose group has <= kZLane anchors
__global__ void zsplit_kernel(ZParams P) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int32_t lo = 0, hi = P.G;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        const int g = P.order[mid];
        if (P.g_start[g + 1] - P.g_start[g] <= kZLane) hi = mid;
        else lo = mid + 1;
    }
    P.lists[0] = lo;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return (uint64_t)hi << 32 | lo;
}

// one wave per group of > kZLane anchors (grid-stride over the list prefix)
__global__ __launch_bounds__(256) void zorder_wave_kernel(ZParams P) {
    const int lane = threadIdx.x & 63;
    const int32_t split = P.lists[0];
    const int nw = (int)(gridDim.x * (blockDim.x >> 6));
    // list entries held per wave (lane i: the i-th pending group) and appended 64 at a time:
    // one returning atomic per listed group on the shared counters serialised (~1 ms per
    // launch over ~10^5 groups, as in query_scan_kernel before)
    int32_t pend[3] = {0, 0, 0};  // merge, mid, big
    int np[3] = {0, 0, 0};
    unsigned long long big_m = 0;  // z entries of this wave's big groups
    int32_t *const lst[3] = {P.merge_list, P.mid_list, P.big_list};
    auto flush = [&](int l) {
        if (np[l] == 0) return;
        int base = 0;
        if (lane == 0) base = atomicAdd(P.lists + (l == 0 ? 3 : l == 1 ? 1 : 2), np[l]);
        base = __shfl(base, 0, 64);
        if (lane < np[l]) lst[l][base + lane] = pend[l];
        np[l] = 0;
    };
    auto push = [&](int l, int g) {
        if (lane == np[l]) pend[l] = g;
        if (++np[l] == 64) flush(l);
    };
    // The wave's groups are w0, w0 + nw, w0 + 2 nw, ...; each round loads the next 64 of them
    // (list entry and bounds, lane r holding group r) in one round trip instead of two dependent
    // ones per group -- most groups are a single chunk of f, so those round trips were half the
    // wave's time.
    for (int wb = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); wb < split; wb += 64 * nw) {
        const int64_t wl = (int64_t)wb + (int64_t)lane * nw;
        int gl = 0;
        int64_t sl = 0, el = 0;
        if (wl < split) {
            gl = P.order[wl];
            sl = P.g_start[gl];
            el = P.g_start[gl + 1];
        }
        const int nr = (int)min((int64_t)64, ((int64_t)split - wb + nw - 1) / nw);  // groups this round
        for (int r = 0; r < nr; r++) {
            const int g = __builtin_amdgcn_readlane(gl, r);
            const int64_t g0 = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int32_t)(sl >> 32), r) << 32 |
                                         (uint32_t)__builtin_amdgcn_readlane((int32_t)sl, r));
            const int64_t n = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int32_t)(el >> 32), r) << 32 |
                                        (uint32_t)__builtin_amdgcn_readlane((int32_t)el, r)) - g0;
            int32_t *rs = P.run_start + (int64_t)g * kZRuns;
            int m = 0, K = 0;  // z entries so far, descents so far (wave-uniform)
            uint64_t last = 0;
            const uint64_t below = (1ull << lane) - 1;
            // kZDepth chunks of f loaded together: a group of tens of thousands of anchors is one
            // wave's serial walk, the launch's tail (one chunk ahead: a round trip per 64 anchors)
            for (int64_t base0 = 0; base0 < n; base0 += 64 * kZDepth) {
                int32_t fc[kZDepth];
#pragma unroll
                for (int d = 0; d < kZDepth; d++) {
                    const int64_t i = base0 + 64 * d + lane;
                    fc[d] = i < n ? P.f[g0 + i] : 0;
                }
#pragma unroll
                for (int d = 0; d < kZDepth; d++) {
                    const int64_t i = base0 + 64 * d + lane;
                    const bool ok = i < n;
                    const int32_t fv = fc[d];
                    const bool z = ok && fv >= P.min_sc;
                    const uint64_t bal = __ballot(z);
                    if (bal == 0) continue;
                    const uint64_t key = (uint64_t)(uint32_t)fv << 32 | (uint32_t)(g0 + i);
                    const uint64_t lower = bal & below;
                    const int pos = m + __popcll(lower);
                    const int prev = lower ? 63 - __clzll((long long)lower) : lane;
                    uint64_t pk = shfl64(key, prev);
                    if (!lower) pk = last;
                    const bool desc = z && pos > 0 && key < pk;
                    const uint64_t dbal = __ballot(desc);
                    if (z) P.z_idx[g0 + pos] = (int32_t)(g0 + i);
                    if (desc) {
                        const int r = K + 1 + __popcll(dbal & below);
                        if (r < kZRuns) rs[r] = pos;
                    }
                    K += __popcll(dbal);
                    m += __popcll(bal);
                    last = shfl64(key, 63 - __clzll((long long)bal));
                }
            }
            const int runs = m > 0 ? K + 1 : 0;
            if (lane == 0) {
                rs[0] = 0;
                P.z_cnt[g] = m;
                P.z_runs[g] = runs;
            }
            if (runs > 1) {
                // only the merge / sort paths read the keys: a group of one run (C4's colinear
                // chains: most of them) writes its order alone, 4 B per z entry instead of 12, and
                // the others write the keys in a second pass over f
                int m2 = 0;
                for (int64_t base0 = 0; base0 < n; base0 += 64 * kZDepth) {
                    int32_t fc[kZDepth];
#pragma unroll
                    for (int d = 0; d < kZDepth; d++) {
                        const int64_t i = base0 + 64 * d + lane;
                        fc[d] = i < n ? P.f[g0 + i] : 0;
                    }
#pragma unroll
                    for (int d = 0; d < kZDepth; d++) {
                        const int64_t i = base0 + 64 * d + lane;
                        const bool z = i < n && fc[d] >= P.min_sc;
                        const uint64_t bal = __ballot(z);
                        if (bal == 0) continue;
                        if (z) P.zkey[g0 + m2 + __popcll(bal & below)] = (uint64_t)(uint32_t)fc[d] << 32 | (uint32_t)(g0 + i);
                        m2 += __popcll(bal);
                    }
                }
            }
            // (wave-uniform conditions)
            if (runs > 1 && runs <= P.max_runs) {
                if (m <= P.zm_lds) {
                    push(0, g);
                } else {  // a long merge is split over blocks (one block walking it was the launch's tail)
                    const int nu = (m + P.zm_unit - 1) / P.zm_unit;
                    int base = 0;
                    if (lane == 0) base = atomicAdd(P.lists + 6, nu);
                    base = __shfl(base, 0, 64);
                    for (int u = lane; u < nu; u += 64) P.mergeu_list[base + u] = (int64_t)g << 32 | (uint32_t)u;
                }
            }
            if (runs > P.max_runs) {
                if (m <= kZs) {
                    push(1, g);
                } else {
                    // list rank only: the radix arrays' offsets are a scan of the counts in rank
                    // order (zbig_count_kernel), since the sorted keys come out rank-major
                    push(2, g);
                    big_m += (unsigned long long)m;
                }
            }
        }
    }
    flush(0), flush(1), flush(2);
    if (lane == 0 && big_m) atomicAdd((unsigned long long *)(P.lists + 4), big_m);
}

// one lane per group of <= kZLane anchors: rank = number of smaller keys
__global__ __launch_bounds__(256) void zorder_lane_kernel(ZParams P) {
    const int32_t w = P.lists[0] + (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (w >= P.G) return;
    const int g = P.order[w];
    const int64_t g0 = P.g_start[g];
    const int n = (int)(P.g_start[g + 1] - g0);
    uint64_t key[kZLane];
#pragma unroll
    for (int j = 0; j < kZLane; j++) {
        const int32_t fv = j < n ? P.f[g0 + j] : 0;
        key[j] = j < n && fv >= P.min_sc ? (uint64_t)(uint32_t)fv << 32 | (uint32_t)(g0 + j) : ~0ull;
    }
    int m = 0;
#pragma unroll
    for (int j = 0; j < kZLane; j++) {
        if (key[j] == ~0ull) continue;
        int r = 0;
#pragma unroll
        for (int k = 0; k < kZLane; k++) r += key[k] < key[j];
        P.z_idx[g0 + r] = (int32_t)(uint32_t)key[j];
        m++;
    }
    P.z_cnt[g] = m;
    P.z_runs[g] = m > 0 ? 1 : 0;  // complete
}

// groups of 2..max_runs ascending runs: merge by ranks, one block per listed group (grid-stride
// over the list; a flat pass over every anchor position read each one's group first).  An
// entry's position is its offset in its own run plus, per other run, the count of smaller keys
// there; a group of up to kZmLds entries is staged in LDS first (real repeats: groups of many
// runs and thousands of entries).  Each thread takes a stripe of consecutive entries: within a
// run the keys ascend, so each other run's count only moves forward from the previous entry's,
// found by an exponential search from there (mostly one compare) instead of a full binary search
// per entry and run; a new run (the key drops) restarts the counts at the run starts.
// entries [qa, qb) of a group of m entries in K runs (rs: K + 1 run bounds)
__device__ __forceinline__ void zmerge_group(const uint64_t *zk, const int32_t *rs, int K, int m, int qa, int qb,
                                             int32_t *out) {
    const int S = (qb - qa + (int)blockDim.x - 1) / (int)blockDim.x;  // entries per thread
    const int q0 = qa + (int)threadIdx.x * S, q1 = min(q0 + S, qb);
    if (q0 >= qb) return;
    int rsr[kZRuns + 1], lo[kZRuns];
#pragma unroll
    for (int k = 0; k <= kZRuns; k++) rsr[k] = k <= K ? rs[k] : m;
    int own = 0, own_s = 0;  // the run of entry q and its start (no dynamic register indexing)
#pragma unroll
    for (int k = 1; k < kZRuns; k++)
        if (k < K && rsr[k] <= q0) own = k, own_s = rsr[k];
    uint64_t prev = ~0ull;
    for (int q = q0; q < q1; q++) {
        const uint64_t key = zk[q];
        const bool restart = key < prev;  // the first entry, or the first of the next run
        prev = key;
        if (restart && q > q0) own++, own_s = q;  // a run start is exactly where the key drops
        int pos = q - own_s;                       // the offset in its own run
#pragma unroll
        for (int k = 0; k < kZRuns; k++) {
            if (k < K && k != own) {
                const int s1 = rsr[k + 1];
                int l = restart ? rsr[k] : lo[k];
                if (l < s1 && zk[l] < key) {  // first entry >= key in (l, s1]: gallop, then bisect
                    int b = 1;
                    while (l + b < s1 && zk[l + b] < key) {
                        l += b;
                        b <<= 1;
                    }
                    int a = l + 1, e = min(l + b, s1);
                    while (a < e) {
                        const int mid = (a + e) >> 1;
                        if (zk[mid] < key) a = mid + 1;
                        else e = mid;
                    }
                    l = a;
                }
                lo[k] = l;
                pos += l - rsr[k];
            }
        }
        out[pos] = (int32_t)(uint32_t)key;
    }
}

__global__ __launch_bounds__(256) void zmerge_kernel(ZParams P) {
    __shared__ uint64_t sk[kZmLds];
    __shared__ int32_t srs[kZRuns + 1];
    const int n_list = P.lists[3], n_units = P.lists[6];
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the lists are final (zorder_wave_kernel ran)
        P.mail[0] = P.lists[2];
        P.mail[1] = *reinterpret_cast<const int64_t *>(P.lists + 4);
    }
    // units of the long merges first (they were the tail), then the staged groups
    for (int w = blockIdx.x; w < n_units + n_list; w += gridDim.x) {
        const bool unit = w < n_units;
        const int64_t uw = unit ? P.mergeu_list[w] : 0;
        const int g = unit ? (int)(uw >> 32) : P.merge_list[w - n_units];
        const int K = P.z_runs[g];
        const int64_t z0 = P.g_start[g];
        const int m = P.z_cnt[g];
        const int32_t *rs = P.run_start + (int64_t)g * kZRuns;
        const uint64_t *zk = P.zkey + z0;
        __syncthreads();  // the previous group's readers are done with sk / srs
        if (threadIdx.x <= K) srs[threadIdx.x] = threadIdx.x < K ? rs[threadIdx.x] : m;
        if (!unit)
            for (int q = threadIdx.x; q < m; q += blockDim.x) sk[q] = zk[q];
        __syncthreads();
        if (unit) {
            const int qa = (int)(uint32_t)uw * P.zm_unit;
            zmerge_group(zk, srs, K, m, qa, min(qa + P.zm_unit, m), P.z_idx + z0);
        } else {
            zmerge_group(sk, srs, K, m, 0, m, P.z_idx + z0);
        }
    }
}

// one block per listed group of <= kZs z entries (grid-stride over the list)
__global__ __launch_bounds__(256) void zsort_block_kernel(ZParams P) {
    __shared__ uint64_t s[kZs];
    const int n_list = P.lists[1];
    for (int w = blockIdx.x; w < n_list; w += gridDim.x) {
        const int g = P.mid_list[w];
        const int64_t z0 = P.g_start[g];
        const int n = P.z_cnt[g];
        int np = 128;
        while (np < n) np <<= 1;
        for (int i = threadIdx.x; i < np; i += 256) s[i] = i < n ? P.zkey[z0 + i] : ~0ull;
        __syncthreads();
        for (int k = 2; k <= np; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = threadIdx.x; i < np; i += 256) {
                    const int ij = i ^ j;
                    if (ij > i) {
                        const uint64_t a = s[i], b = s[ij];
                        if (((i & k) == 0) == (a > b)) {
                            s[i] = b;
                            s[ij] = a;
                        }
                    }
                }
                __syncthreads();
            }
        for (int i = threadIdx.x; i < n; i += 256) P.z_idx[z0 + i] = (int32_t)(uint32_t)s[i];
        __syncthreads();
    }
}

// z entries of each large group, in list-rank order (scanned into big_off)
__global__ void zbig_count_kernel(ZParams P, int32_t n_big, uint32_t *cnt) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_big) cnt[r] = (uint32_t)P.z_cnt[P.big_list[r]];
}

// entries of the large groups, list-major: key = rank << 32 | f, value = idx; group r's
// entries start at big_off[r] both before and after the sort (offsets ascend with the rank)
__global__ void zbig_gather_kernel(ZParams P, uint64_t *skey, uint32_t *sval) {
    const int r = blockIdx.x, g = P.big_list[r];
    const int64_t z0 = P.g_start[g], n = P.z_cnt[g], o = P.big_off[r];
    for (int64_t t = threadIdx.x; t < n; t += blockDim.x) {
        const uint64_t k = P.zkey[z0 + t];
        skey[o + t] = (uint64_t)r << 32 | (k >> 32);
        sval[o + t] = (uint32_t)k;
    }
}

__global__ void zbig_scatter_kernel(ZParams P, const uint32_t *sval) {
    const int r = blockIdx.x, g = P.big_list[r];
    const int64_t z0 = P.g_start[g], n = P.z_cnt[g], o = P.big_off[r];
    for (int64_t t = threadIdx.x; t < n; t += blockDim.x) P.z_idx[z0 + t] = (int32_t)sval[o + t];
}

// chain list entries: (key = first anchor index) -> sorted
__global__ void chain_list_kernel(const int64_t *g_start, const int32_t *n_chains, const int64_t *c_pos, int32_t G,
                                  const uint64_t *chain_u, const int64_t *chain_first, const int32_t *chain_ids,
                                  uint64_t *ckey, uint64_t *cu, int64_t *cfirst) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int64_t g0 = g_start[g];
    int64_t o = c_pos[g];
    for (int c = 0; c < n_chains[g]; c++, o++) {
        const int64_t fo = chain_first[g0 + c];
        ckey[o] = (uint64_t)chain_ids[fo + (uint32_t)chain_u[g0 + c] - 1];  // stored end -> start
        cu[o] = chain_u[g0 + c];
        cfirst[o] = fo;
    }
}

// anchors per chain in chain order; with a long join (qflag and cnt2 given), the chains of
// flagged queries count into cnt2 instead: they take no slots, their anchors are only marked
__global__ void chain_cnt_kernel(const uint64_t *cu, const uint32_t *cq, const uint32_t *qflag, int64_t n, uint32_t *cnt,
                                 uint32_t *cnt2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = (uint32_t)cu[i];
    const bool fl = qflag && qflag[cq[i]];
    cnt[i] = fl ? 0u : m;
    if (cnt2) cnt2[i] = fl ? m : 0u;
}

// long join, first pass (map.c's rmq rescue): a query is re-chained when it has more than one
// chain and its first chain (compact order) leaves too much of it uncovered -- read from the
// chain list
__global__ void rechain_flag_kernel(const uint32_t *ay, const int32_t *chain_ids, const uint64_t *cu, const int64_t *cfirst,
                                    const int64_t *qc, const int64_t *qlen, int n_q, int rescue_size, float rescue_ratio,
                                    uint32_t *flag) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    const int64_t c0 = qc[q], nc = qc[q + 1] - c0;
    uint32_t f = 0;
    if (nc > 1) {
        const int32_t m = (int32_t)cu[c0];
        const int64_t fo = cfirst[c0];  // backtrack stores end -> start
        const int32_t st = (int32_t)ay[chain_ids[fo + m - 1]], en = (int32_t)ay[chain_ids[fo]];
        const int32_t ql = (int32_t)qlen[q];
        if (ql - (en - st) > rescue_size || (float)(en - st) > __fmul_rn((float)ql, rescue_ratio)) f = 1;
    }
    flag[q] = f;
}

// per-query anchor offsets in chain order: the offset of the query's first chain
__global__ void chain_qb_kernel(const int64_t *qc, const int64_t *bpos, int64_t n_chain, int64_t nb, int n_q, int64_t *qb) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > n_q) return;
    const int64_t c = qc[q];
    qb[q] = c < n_chain ? bpos[c] : nb;
}

// Long-join anchors: the first pass's chain anchors (t == 2 after the backtrack) of the
// flagged queries.  Thread l of a 4096-anchor tile decides anchors [16 l, 16 l + 16) of the
// tile (their 16 byte marks in one 16-byte load; the query of the first by a binary search
// over the query offsets, then stepping over the few query starts inside the 16).
__device__ __forceinline__ uint32_t keep_bits16(const uint8_t *t, int64_t n, const uint32_t *qflag, const int64_t *qoff,
                                                int n_q, int64_t e0) {
    if (e0 >= n) return 0u;
    int lo = 0, hi = n_q - 1;  // last q with qoff[q] <= e0
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (qoff[mid] <= e0) lo = mid;
        else hi = mid - 1;
    }
    int q = lo;
    int64_t qend = qoff[q + 1];
    uint32_t v[4] = {0, 0, 0, 0};  // mark u: byte u & 3 of v[u >> 2]
    if (e0 + 16 <= n) {
        const uint4 w = *reinterpret_cast<const uint4 *>(t + e0);  // e0 is a multiple of 16
        v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
    } else {
#pragma unroll
        for (int u = 0; u < 16; u++) v[u >> 2] |= (e0 + u < n ? (uint32_t)t[e0 + u] : 0u) << (8 * (u & 3));
    }
    uint32_t bits = 0, fl = qflag[q];
#pragma unroll
    for (int u = 0; u < 16; u++) {
        while (e0 + u >= qend && q + 1 < n_q) {  // a query starts here
            q++;
            qend = qoff[q + 1];
            fl = qflag[q];
        }
        bits |= (uint32_t)((v[u >> 2] >> (8 * (u & 3)) & 0xffu) == 2u && fl != 0) << u;
    }
    return bits;
}

// (also each tile's last kept anchor, or -1: the compaction's group heads compare a tile's
// first kept anchor with the one before it)
__global__ __launch_bounds__(256) void mark_count_kernel(const uint8_t *t, int64_t n, const uint32_t *qflag,
                                                         const int64_t *qoff, int n_q, uint32_t *cnt, int64_t *last_kept) {
    __shared__ uint32_t ws[4];
    __shared__ int64_t wl[4];
    const int64_t e0 = (int64_t)blockIdx.x * 4096 + threadIdx.x * 16;
    const uint32_t kb = keep_bits16(t, n, qflag, qoff, n_q, e0);
    uint32_t c = __popc(kb);
    long long l = kb ? e0 + 31 - __clz((int)kb) : -1;
    for (int o = 32; o > 0; o >>= 1) {
        c += __shfl_xor((int)c, o, 64);
        l = max(l, __shfl_xor(l, o, 64));
    }
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c, wl[threadIdx.x >> 6] = l;
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
        last_kept[blockIdx.x] = max(max(wl[0], wl[1]), max(wl[2], wl[3]));
    }
}

// stable compaction of the kept anchors (x, y): the first-pass set is sorted by (query, x,
// y), so its kept subsequence is the long join's sorted anchor set -- no re-sort.  The keep
// bits are decided per 16 consecutive anchors (as in the count) into LDS; rows of 256
// anchors are then written lanes striped (coalesced), positions by ballot counts.
// The output's group heads (x >> 32 differs from the previous kept anchor's) go into its
// bitmap ohb (zeroed): the previous kept anchor is a lower lane of the same 64-anchor chunk
// (shuffle), else the last kept one of an earlier chunk of the tile (LDS), else the last kept
// anchor of an earlier tile (last_kept, from the count).
__global__ __launch_bounds__(256) void mark_compact_kernel(const uint8_t *t, int64_t n, const uint32_t *qflag,
                                                           const int64_t *qoff, int n_q, const int64_t *tile_off,
                                                           const int64_t *last_kept, const uint64_t *ax, const uint32_t *ay,
                                                           uint64_t *ox, uint32_t *oy, uint32_t *ohb, uint32_t *ox32) {
    __shared__ uint32_t rc[64];       // kept per (row, wave), row-major
    __shared__ uint32_t nk[64];       // the same counts (rc becomes their exclusive scan)
    __shared__ uint32_t lx[64];       // x >> 32 of each (row, wave) chunk's last kept anchor
    __shared__ uint16_t kb[256];      // keep bits of anchors [16 l, 16 l + 16) of the tile
    const int64_t t0 = (int64_t)blockIdx.x * 4096;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    kb[threadIdx.x] = (uint16_t)keep_bits16(t, n, qflag, qoff, n_q, t0 + threadIdx.x * 16);
    __syncthreads();
    bool m[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int r = j * 256 + threadIdx.x;  // tile-relative anchor
        m[j] = (kb[r >> 4] >> (r & 15)) & 1;
        const uint64_t b = __ballot(m[j]);
        if (lane == 0) rc[j * 4 + w] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    uint32_t v = 0, inc = 0;
    if (w == 0) nk[lane] = rc[lane];
    if (w == 0) {  // wave 0: exclusive scan of the 64 counts in element order
        v = rc[lane];
        inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
            if (lane >= d) inc += o;
        }
    }
    __syncthreads();
    if (w == 0) rc[lane] = inc - v;
    __syncthreads();
    const int64_t base = tile_off[blockIdx.x];
    uint32_t xh[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint64_t b = __ballot(m[j]);
        xh[j] = 0;
        if (m[j]) {
            const int64_t e = t0 + j * 256 + threadIdx.x;
            const int64_t o = base + rc[j * 4 + w] + __popcll(b & ((1ull << lane) - 1));
            const uint64_t xv = ax[e];
            xh[j] = (uint32_t)(xv >> 32);
            ox[o] = xv;
            ox32[o] = (uint32_t)xv;
            oy[o] = ay[e];
        }
        if (b && lane == 63 - __clzll((long long)b)) lx[j * 4 + w] = xh[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint64_t b = __ballot(m[j]);
        const uint64_t below = b & ((1ull << lane) - 1);
        const int src = below ? 63 - __clzll((long long)below) : lane;
        const uint32_t xp = (uint32_t)__shfl((int)xh[j], src, 64);
        if (m[j]) {
            bool hd;
            if (below) {
                hd = xp != xh[j];
            } else {  // the chunk's first kept anchor
                int c = j * 4 + w - 1;
                while (c >= 0 && nk[c] == 0) --c;
                if (c >= 0) {
                    hd = lx[c] != xh[j];
                } else {  // the tile's first: the last kept anchor of an earlier tile
                    int64_t tt = (int64_t)blockIdx.x - 1;
                    while (tt >= 0 && last_kept[tt] < 0) --tt;
                    hd = tt < 0 || (uint32_t)(ax[last_kept[tt]] >> 32) != xh[j];
                }
            }
            if (hd) {
                const int64_t o = base + rc[j * 4 + w] + __popcll(below);
                atomicOr(ohb + (o >> 5), 1u << (o & 31));
            }
        }
    }
}

// query of each chain (from the sorted first-anchor key, via the anchor query offsets)
__global__ void chain_query_kernel(const uint64_t *ckey, int64_t n, const int64_t *a_off, int n_q, uint32_t *cq) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n) cq[c] = (uint32_t)upper_idx(a_off, n_q, (int64_t)ckey[c]);
}

__global__ void count_per_query_kernel(const uint32_t *cq, int64_t n, int n_q, int64_t *q_first) {
    // q_first[q] = first chain index of query q (lower bound), q_first[n_q] = n
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n) return;
    const int64_t qp = p == 0 ? -1 : (int64_t)cq[p - 1];
    const int64_t qc = p == n ? (int64_t)n_q : (int64_t)cq[p];
    for (int64_t q = qp + 1; q <= qc; q++) q_first[q] = p;
}

// ---------------------------------------------------------------- stages
// (query, strand, target) runs of an anchor set
struct Groups {
    DevBuf g_start;  // G + 1 group starts, g_start[G] = n
    DevBuf qfirst;   // per group: it starts its query's anchor array (the krmq index-0 quirk)
    int64_t G = 0;
};

// the groups of at least min_cnt anchors, biggest first
struct WorkList {
    DevBuf order;   // group ids by descending size (int32): the first n_work are the work groups
    DevBuf zlists;  // the z-order stage's list counters, zeroed by group_size_kernel
    int64_t n_work = 0, largest = 0;
};

struct DpArgs {
    int max_dist, max_dist_inner, bw, max_chn_skip, cap_rmq_size;
    float pen_gap, pen_skip;
    int min_cnt;
};

// backtrack order: group g's anchors with f >= min_sc, ascending (f, idx), at idx[g_start[g] + [0, cnt[g])]
struct ZOrder {
    DevBuf idx, cnt;
};

// launch_backtrack's output: per group its chains (score | count, first slot) and their
// anchors, each chain end -> start, inside the group's own anchor range
struct Backtrack {
    DevBuf ids, u, first, n_chains;
};

// the head bitmap and x's low words of a set whose writer left them out
static int derive_heads(hymet_ctx *ctx, AnchorSet &A) {
    const int64_t n = A.n;
    if (!A.has_hb) {
        HY_HIP(A.hb.alloc(head_bits_bytes(n), ctx->stream));
        LAUNCH1(head_bits_x_kernel, n, A.ax.as<uint64_t>(), n, A.hb.as<uint64_t>());
        A.has_hb = true;
    }
    if (!A.has_x32) {
        HY_HIP(A.ax32.alloc(4 * (size_t)n, ctx->stream));
        LAUNCH1(x_low_kernel, n, A.ax.as<uint64_t>(), n, A.ax32.as<uint32_t>());
        A.has_x32 = true;
    }
    return HYMET_OK;
}

// groups from the set's head bitmap by tiles: count, scan of the tile counts, write
static int build_groups(hymet_ctx *ctx, const AnchorSet &A, int n_q, Groups &Gr) {
    const int64_t n = A.n, ntile = cdiv(n, kGTile);
    DevBuf tcnt, toff;
    HY_HIP(tcnt.alloc(4 * (size_t)(ntile + 1), ctx->stream));
    HY_HIP(toff.alloc(8 * (size_t)(ntile + 1), ctx->stream));
    hipLaunchKernelGGL(group_heads_count_kernel, dim3((unsigned)ntile), dim3(256), 0, ctx->stream, A.hb.as<uint32_t>(), n,
                       A.d_off.as<int64_t>(), n_q, tcnt.as<uint32_t>());
    HY_CHECK_LAUNCH("group_heads_count_kernel");
    int rc = exclusive_scan_u32_i64(ctx, tcnt.as<uint32_t>(), toff.as<int64_t>(), ntile, &Gr.G);
    if (rc) return rc;
    HY_HIP(Gr.g_start.alloc(8 * (size_t)(Gr.G + 1), ctx->stream));
    HY_HIP(Gr.qfirst.alloc((size_t)Gr.G, ctx->stream));
    hipLaunchKernelGGL(group_heads_write_kernel, dim3((unsigned)ntile), dim3(256), 0, ctx->stream, A.hb.as<uint32_t>(), n,
                       A.d_off.as<int64_t>(), n_q, toff.as<int64_t>(), Gr.g_start.as<int64_t>(), Gr.qfirst.as<uint8_t>(), Gr.G);
    HY_CHECK_LAUNCH("group_heads_write_kernel");
    return HYMET_OK;
}

// work list: the groups sorted by descending size (non-work groups last), the work groups
// counted on the host; the chaining kernel packs local predecessor indices in 24 bits
static int build_work_list(hymet_ctx *ctx, const Groups &Gr, int min_cnt, WorkList &W) {
    const int64_t G = Gr.G;
    DevBuf skey, sidx, swork, skey2, sidx2, wpos;
    for (DevBuf *b : {&skey, &sidx, &swork, &skey2, &sidx2}) HY_HIP(b->alloc(4 * (size_t)G, ctx->stream));
    HY_HIP(W.zlists.alloc(32, ctx->stream));
    LAUNCH1(group_size_kernel, std::max<int64_t>(G, 8), Gr.g_start.as<int64_t>(), (int32_t)G, min_cnt, skey.as<uint32_t>(),
            sidx.as<uint32_t>(), swork.as<uint32_t>(), (uint8_t *)nullptr, W.zlists.as<int32_t>());
    int rc = scan_flags(ctx, swork.as<uint32_t>(), G, wpos, &W.n_work);
    if (rc) return rc;
    uint32_t *kp = skey.as<uint32_t>(), *ka = skey2.as<uint32_t>(), *vp = sidx.as<uint32_t>(), *va = sidx2.as<uint32_t>();
    rc = sort_pairs(ctx, kp, ka, vp, va, G, 0, 16, "radix_sort_groups");
    if (rc) return rc;
    LAUNCH1(max_group_kernel, 1, Gr.g_start.as<int64_t>(), (const int32_t *)vp, (int32_t)G, mb_dev(ctx, kMbGmax));
    HY_HIP(hipStreamSynchronize(ctx->stream));
    W.largest = mb_read(ctx, kMbGmax);
    HY_ARG(W.largest < (1ll << 24) - 1, "chaining: an anchor group exceeds 2^24 anchors");
    W.order.swap(vp == sidx.as<uint32_t>() ? sidx : sidx2);
    return HYMET_OK;
}

// f / p of every anchor: the chaining kernels write those of the work groups; the anchors of
// groups of fewer than min_cnt anchors get f = 0, p = -1 from nonwork_fp_kernel instead of
// memsets of all n.  The walk's stamps go to the context's stamp scratch (zero before and
// after)
static int chain_dp(hymet_ctx *ctx, const DpArgs &a, const AnchorSet &A, const Groups &Gr, const WorkList &W, DevBuf &f,
                    DevBuf &p) {
    HY_HIP(f.alloc(4 * (size_t)A.n, ctx->stream));
    HY_HIP(p.alloc(4 * (size_t)A.n, ctx->stream));
    int32_t *stamp = nullptr;
    HY_HIP(stamp_scratch(ctx, A.n, &stamp));
    LAUNCH1(nonwork_fp_kernel, Gr.G, Gr.g_start.as<int64_t>(), (int32_t)Gr.G, a.min_cnt, f.as<int32_t>(), p.as<int32_t>());
    return launch_chain(ctx, A.ax32.as<int32_t>(), A.ay.as<uint32_t>(), A.span, Gr.g_start.as<int64_t>(), Gr.qfirst.as<uint8_t>(),
                        W.order.as<int32_t>(), (int32_t)W.n_work, f.as<int32_t>(), p.as<int32_t>(), stamp, a.max_dist,
                        a.max_dist_inner, a.bw, a.max_chn_skip, a.cap_rmq_size, a.pen_gap, a.pen_skip, A.n, Gr.G);
}

// z = anchors with f >= min_sc ordered by (group, f, idx), inside each group's range
static int z_order(hymet_ctx *ctx, int min_sc, const DevBuf &f, int64_t n, const Groups &Gr, const WorkList &W, ZOrder &Z) {
    const int64_t G = Gr.G;
    DevBuf zkey, z_runs, run_start, merge_list, mergeu_list, mid_list, big_list, big_off;
    HY_HIP(zkey.alloc(8 * (size_t)n, ctx->stream));
    HY_HIP(Z.idx.alloc(4 * (size_t)n, ctx->stream));
    HY_HIP(Z.cnt.alloc(4 * (size_t)G, ctx->stream));
    HY_HIP(z_runs.alloc(4 * (size_t)G, ctx->stream));
    HY_HIP(run_start.alloc(4 * (size_t)G * kZRuns, ctx->stream));
    HY_HIP(merge_list.alloc(4 * (size_t)G, ctx->stream));
    // HYMET_ZM_LDS / HYMET_ZM_UNIT (tests): stage merge groups up to that many entries, split
    // the others into units of that many; HYMET_Z_RUNS (tests): merge groups of at most that
    // many runs, sort the others
    const int zm_lds = (int)env_int("HYMET_ZM_LDS", kZmLds, 0, kZmLds);
    const int zm_unit = (int)env_int("HYMET_ZM_UNIT", kZmUnit, 1, INT32_MAX);
    const int max_runs = (int)env_int("HYMET_Z_RUNS", kZRuns, 1, kZRuns);
    HY_HIP(mergeu_list.alloc(8 * (size_t)(n / zm_unit + G + 16), ctx->stream));  // >= sum of cdiv(m, unit)
    HY_HIP(mid_list.alloc(4 * (size_t)G, ctx->stream));
    HY_HIP(big_list.alloc(4 * (size_t)G, ctx->stream));
    HY_HIP(big_off.alloc(8 * (size_t)G, ctx->stream));
    ProfScope _ps(ctx, "mm_z_order", 16.0 * (double)n);  // f read, key + idx written (z entries <= anchors)
    ZParams P{f.as<int32_t>(), Gr.g_start.as<int64_t>(), W.order.as<int32_t>(), (int32_t)G, min_sc,
              max_runs, zm_lds, zm_unit, zkey.as<uint64_t>(), Z.idx.as<int32_t>(), Z.cnt.as<int32_t>(), z_runs.as<int32_t>(),
              run_start.as<int32_t>(), W.zlists.as<int32_t>(), merge_list.as<int32_t>(), mergeu_list.as<int64_t>(),
              mid_list.as<int32_t>(), big_list.as<int32_t>(),
              big_off.as<int64_t>(), mb_dev(ctx, kMbZBig)};
    hipLaunchKernelGGL(zsplit_kernel, dim3(1), dim3(64), 0, ctx->stream, P);
    HY_CHECK_LAUNCH("zsplit_kernel");
    const int64_t nwb = std::min<int64_t>(cdiv(G, 4), (int64_t)ctx->n_cu * 8);
    hipLaunchKernelGGL(zorder_wave_kernel, dim3((unsigned)std::max<int64_t>(nwb, 1)), dim3(256), 0, ctx->stream, P);
    HY_CHECK_LAUNCH("zorder_wave_kernel");
    LAUNCH1(zorder_lane_kernel, G, P);
    const int64_t nb = std::min<int64_t>(G, (int64_t)ctx->n_cu * 8);
    hipLaunchKernelGGL(zmerge_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, P);
    HY_CHECK_LAUNCH("zmerge_kernel");
    hipLaunchKernelGGL(zsort_block_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, P);
    HY_CHECK_LAUNCH("zsort_block_kernel");
    HY_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t n_big = mb_read(ctx, kMbZBig), nz_big = mb_read(ctx, kMbZBigTotal);
    if (n_big == 0) return HYMET_OK;
    // the groups too large for the block sort: one global radix sort over all of them
    DevBuf bcnt;
    HY_HIP(bcnt.alloc(4 * (size_t)(n_big + 1), ctx->stream));
    LAUNCH1(zbig_count_kernel, n_big, P, (int32_t)n_big, bcnt.as<uint32_t>());
    int64_t nz_scan = 0;
    int rc = exclusive_scan_u32_i64(ctx, bcnt.as<uint32_t>(), big_off.as<int64_t>(), n_big, &nz_scan);
    if (rc) return rc;
    if (nz_scan != nz_big) return hymet::fail(HYMET_E_INTERNAL, "hymet_mm_map: z list count mismatch");
    DevBuf sk, sk2, sv, sv2;
    HY_HIP(sk.alloc(8 * (size_t)nz_big, ctx->stream));
    HY_HIP(sk2.alloc(8 * (size_t)nz_big, ctx->stream));
    HY_HIP(sv.alloc(4 * (size_t)nz_big, ctx->stream));
    HY_HIP(sv2.alloc(4 * (size_t)nz_big, ctx->stream));
    hipLaunchKernelGGL(zbig_gather_kernel, dim3((unsigned)n_big), dim3(256), 0, ctx->stream, P, sk.as<uint64_t>(),
                       sv.as<uint32_t>());
    HY_CHECK_LAUNCH("zbig_gather_kernel");
    uint64_t *kp = sk.as<uint64_t>(), *ka = sk2.as<uint64_t>();
    uint32_t *vp = sv.as<uint32_t>(), *va = sv2.as<uint32_t>();
    rc = sort_pairs(ctx, kp, ka, vp, va, nz_big, 0, 32 + bits_for(n_big), "radix_sort_z_big");
    if (rc) return rc;
    hipLaunchKernelGGL(zbig_scatter_kernel, dim3((unsigned)n_big), dim3(256), 0, ctx->stream, P, (const uint32_t *)vp);
    HY_CHECK_LAUNCH("zbig_scatter_kernel");
    return HYMET_OK;
}

static int backtrack(hymet_ctx *ctx, const hymet_mm_opt *opt, int bw, int64_t n, const Groups &Gr, const WorkList &W,
                     const DevBuf &f, const DevBuf &p, DevBuf &t, const ZOrder &Z, Backtrack &B) {
    HY_HIP(B.ids.alloc(4 * (size_t)n, ctx->stream));
    HY_HIP(B.u.alloc(8 * (size_t)n, ctx->stream));
    HY_HIP(B.first.alloc(8 * (size_t)n, ctx->stream));
    HY_HIP(B.n_chains.alloc(4 * (size_t)Gr.G, ctx->stream));
    return launch_backtrack(ctx, Gr.g_start.as<int64_t>(), f.as<int32_t>(), p.as<int32_t>(), t.as<uint8_t>(), Z.cnt.as<int32_t>(),
                            Z.idx.as<int32_t>(), (int32_t)Gr.G, W.order.as<int32_t>(), (int32_t)W.n_work, opt->min_cnt,
                            opt->min_chain_score, bw, B.ids.as<int32_t>(), B.u.as<uint64_t>(), B.first.as<int64_t>(),
                            B.n_chains.as<int32_t>(), n);
}

// chain list sorted by first anchor index (compact_a order): C.cu, each chain's query C.cq,
// the per-query chain offsets C.d_qc, and cfirst (each chain's first slot in B.ids)
static int chain_list(hymet_ctx *ctx, const AnchorSet &A, int n_q, const Groups &Gr, const Backtrack &B, ChainSet &C,
                      DevBuf &cfirst) {
    const int64_t G = Gr.G;
    DevBuf cpos;
    int64_t NC = 0;
    int rc = scan_flags(ctx, (const uint32_t *)B.n_chains.p, G, cpos, &NC);
    if (rc) return rc;
    C.n_chain = NC;
    DevBuf ckey, cu, cf;
    HY_HIP(ckey.alloc(8 * (size_t)(NC + 1), ctx->stream));
    HY_HIP(cu.alloc(8 * (size_t)(NC + 1), ctx->stream));
    HY_HIP(cf.alloc(8 * (size_t)(NC + 1), ctx->stream));
    LAUNCH1(chain_list_kernel, G, Gr.g_start.as<int64_t>(), B.n_chains.as<int32_t>(), cpos.as<int64_t>(), (int32_t)G,
            B.u.as<uint64_t>(), B.first.as<int64_t>(), B.ids.as<int32_t>(), ckey.as<uint64_t>(), cu.as<uint64_t>(),
            cf.as<int64_t>());
    // sort chains by first anchor: pairs (key, perm) then gather
    DevBuf perm, perm2, ckeyb;
    HY_HIP(perm.alloc(4 * (size_t)(NC + 1), ctx->stream));
    HY_HIP(perm2.alloc(4 * (size_t)(NC + 1), ctx->stream));
    HY_HIP(ckeyb.alloc(8 * (size_t)(NC + 1), ctx->stream));
    LAUNCH1(iota_u32_kernel, NC, perm.as<uint32_t>(), NC);
    uint64_t *ck = ckey.as<uint64_t>(), *cka = ckeyb.as<uint64_t>();
    uint32_t *pp = perm.as<uint32_t>(), *ppa = perm2.as<uint32_t>();
    rc = sort_pairs(ctx, ck, cka, pp, ppa, NC, 0, bits_for(A.n), "radix_sort_chains");
    if (rc) return rc;
    HY_HIP(C.cu.alloc(8 * (size_t)(NC + 1), ctx->stream));
    HY_HIP(cfirst.alloc(8 * (size_t)(NC + 1), ctx->stream));
    LAUNCH1(gather_kernel<uint64_t>, NC, cu.as<uint64_t>(), pp, C.cu.as<uint64_t>(), NC);
    LAUNCH1(gather_kernel<int64_t>, NC, cf.as<int64_t>(), pp, cfirst.as<int64_t>(), NC);
    // per-query chain offsets
    HY_HIP(C.cq.alloc(4 * (size_t)(NC + 1), ctx->stream));
    LAUNCH1(chain_query_kernel, NC, ck, NC, A.d_off.as<int64_t>(), n_q, C.cq.as<uint32_t>());
    HY_HIP(C.d_qc.alloc(8 * (size_t)(n_q + 1), ctx->stream));
    hipLaunchKernelGGL(count_per_query_kernel, dim3((unsigned)cdiv(NC + 1, 256)), dim3(256), 0, ctx->stream,
                       C.cq.as<uint32_t>(), NC, n_q, C.d_qc.as<int64_t>());
    HY_CHECK_LAUNCH("count_per_query_kernel");
    return HYMET_OK;
}

// Where every chain's anchors go in chain order (C.cboff, C.d_qb), and the long join's
// hand-over: the re-chained queries (lj->flag) from the chain list; their chains take no
// slots, and their anchor counts (lj->qb2, lj->n2) and the backtrack's marks t (lj->mark) go
// to the long join instead
static int chain_layout(hymet_ctx *ctx, const AnchorSet &A, int n_q, const DevBuf &chain_ids, const DevBuf &cfirst,
                        ChainSet &C, LeanJoin *lj, DevBuf &t) {
    const int64_t NC = C.n_chain;
    DevBuf ccnt, ccnt2;
    HY_HIP(ccnt.alloc(4 * (size_t)(NC + 1), ctx->stream));
    if (lj) {
        HY_HIP(lj->flag.alloc(4 * (size_t)n_q, ctx->stream));
        LAUNCH1(rechain_flag_kernel, n_q, A.ay.as<uint32_t>(), chain_ids.as<int32_t>(), C.cu.as<uint64_t>(),
                cfirst.as<int64_t>(), C.d_qc.as<int64_t>(), lj->qlen, n_q, lj->rescue_size, lj->rescue_ratio,
                lj->flag.as<uint32_t>());
        HY_HIP(ccnt2.alloc(4 * (size_t)(NC + 1), ctx->stream));
    }
    // anchors of every chain (but those only marked) in chain order
    LAUNCH1(chain_cnt_kernel, NC, C.cu.as<uint64_t>(), C.cq.as<uint32_t>(), lj ? lj->flag.as<uint32_t>() : nullptr, NC,
            ccnt.as<uint32_t>(), lj ? ccnt2.as<uint32_t>() : nullptr);
    int64_t NB = 0;
    int rc = scan_flags(ctx, ccnt.as<uint32_t>(), NC, C.cboff, &NB);
    if (rc) return rc;
    C.n_anchor = NB;
    HY_HIP(C.d_qb.alloc(8 * (size_t)(n_q + 1), ctx->stream));
    LAUNCH1(chain_qb_kernel, n_q + 1, C.d_qc.as<int64_t>(), C.cboff.as<int64_t>(), NC, NB, n_q, C.d_qb.as<int64_t>());
    if (lj) {
        DevBuf boff2;
        rc = scan_flags(ctx, ccnt2.as<uint32_t>(), NC, boff2, &lj->n2);
        if (rc) return rc;
        // the backtrack left t == 2 on every kept chain's anchors: the long join selects
        // those of its queries straight from t (no pass over the chains)
        lj->mark.swap(t);
        HY_HIP(lj->qb2.alloc(8 * (size_t)(n_q + 1), ctx->stream));
        LAUNCH1(chain_qb_kernel, n_q + 1, C.d_qc.as<int64_t>(), boff2.as<int64_t>(), NC, lj->n2, n_q, lj->qb2.as<int64_t>());
    }
    return HYMET_OK;
}

}  // namespace

int chain_set(hymet_ctx *ctx, const hymet_mm_opt *opt, float pen_gap, float pen_skip, int bw, AnchorSet &A, int n_q,
              ChainSet &C, LeanJoin *lj) {
    const int64_t n = A.n;
    HY_ARG(n >= 0 && n < INT32_MAX, "chain_set: an anchor set of 2^31 anchors or more (32-bit chain links)");
    C.ax = A.ax.as<uint64_t>(), C.ay = A.ay.as<uint32_t>(), C.span = A.span;
    if (n == 0) {
        HY_HIP(C.d_qc.alloc(8 * (size_t)(n_q + 1), ctx->stream));
        HY_HIP(C.d_qb.alloc(8 * (size_t)(n_q + 1), ctx->stream));
        HY_HIP(hipMemsetAsync(C.d_qc.p, 0, 8 * (size_t)(n_q + 1), ctx->stream));
        HY_HIP(hipMemsetAsync(C.d_qb.p, 0, 8 * (size_t)(n_q + 1), ctx->stream));
        return HYMET_OK;
    }
    int rc = derive_heads(ctx, A);
    if (rc) return rc;
    C.ax32 = A.ax32.as<uint32_t>();
    Groups Gr;
    rc = build_groups(ctx, A, n_q, Gr);
    if (rc) return rc;
    // t, the backtrack's marks (one byte per anchor, + 16 for the long join's 16-byte loads), is
    // cleared by a fill here, not by the chaining kernels as they decide each anchor: the extra
    // store made the first-pass wave kernel ~3 % slower and the fill overlaps the other mapping
    // stream (profiles/r06_tzero/).  lchain.c's stamps during the DP are not in t: they live in
    // the context's stamp scratch (chain_dp)
    DevBuf t;
    HY_HIP(t.alloc((size_t)n + 16, ctx->stream));
    HY_HIP(hipMemsetAsync(t.p, 0, (size_t)n + 16, ctx->stream));
    WorkList W;
    rc = build_work_list(ctx, Gr, opt->min_cnt, W);
    if (rc) return rc;
    if (env_flag("HYMET_CHAIN_STATS"))  // profiling: tail size per launch
        fprintf(stderr, "[chain] bw %d anchors %lld groups %lld work %lld largest %lld\n", bw, (long long)n, (long long)Gr.G,
                (long long)W.n_work, (long long)W.largest);
    DevBuf f, p;
    rc = chain_dp(ctx, DpArgs{opt->max_gap, opt->rmq_inner_dist, bw, opt->max_chain_skip, opt->rmq_size_cap, pen_gap, pen_skip,
                              opt->min_cnt}, A, Gr, W, f, p);
    if (rc) return rc;
    ZOrder Z;
    rc = z_order(ctx, opt->min_chain_score, f, n, Gr, W, Z);
    if (rc) return rc;
    Backtrack B;
    rc = backtrack(ctx, opt, bw, n, Gr, W, f, p, t, Z, B);
    if (rc) return rc;
    DevBuf cfirst;
    rc = chain_list(ctx, A, n_q, Gr, B, C, cfirst);
    if (rc) return rc;
    rc = chain_layout(ctx, A, n_q, B.ids, cfirst, C, lj, t);
    if (rc) return rc;
    // regions and chain statistics read the chains in place
    C.ids.swap(B.ids);
    C.cfirst.swap(cfirst);
    return HYMET_OK;
}

// the anchors of S1 with mark == 2 in flagged queries, compacted in S1's order into S2
// (expect: their count as the caller knows it, or -1)
static int compact_marked(hymet_ctx *ctx, const AnchorSet &S1, const uint8_t *mark, const uint32_t *flag, int n_q,
                          int64_t expect, AnchorSet &S2) {
    hipStream_t st = ctx->stream;
    const int64_t n1 = S1.n, nt = cdiv(n1, 4096);
    DevBuf tcnt, toff, tlast;
    HY_HIP(tcnt.alloc(4 * (size_t)(nt + 1), st));
    HY_HIP(toff.alloc(8 * (size_t)(nt + 1), st));
    HY_HIP(tlast.alloc(8 * (size_t)(nt + 1), st));
    hipLaunchKernelGGL(mark_count_kernel, dim3((unsigned)nt), dim3(256), 0, st, mark, n1, flag,
                       S1.d_off.as<int64_t>(), n_q, tcnt.as<uint32_t>(), tlast.as<int64_t>());
    HY_CHECK_LAUNCH("mark_count_kernel");
    int64_t A2 = 0;
    int rc = exclusive_scan_u32_i64(ctx, tcnt.as<uint32_t>(), toff.as<int64_t>(), nt, &A2);
    if (rc) return rc;
    if (expect >= 0 && A2 != expect) return hymet::fail(HYMET_E_INTERNAL, "hymet_mm_map: long-join anchor count mismatch");
    HY_HIP(S2.ax.alloc(8 * (size_t)(A2 + 1), st));
    HY_HIP(S2.ay.alloc(4 * (size_t)(A2 + 1), st));
    HY_HIP(S2.hb.alloc(head_bits_bytes(A2), st));
    HY_HIP(S2.ax32.alloc(4 * (size_t)(A2 + 1), st));
    HY_HIP(hipMemsetAsync(S2.hb.p, 0, head_bits_bytes(A2), st));
    hipLaunchKernelGGL(mark_compact_kernel, dim3((unsigned)nt), dim3(256), 0, st, mark, n1, flag,
                       S1.d_off.as<int64_t>(), n_q, toff.as<int64_t>(), tlast.as<int64_t>(), S1.ax.as<uint64_t>(),
                       S1.ay.as<uint32_t>(), S2.ax.as<uint64_t>(), S2.ay.as<uint32_t>(), S2.hb.as<uint32_t>(),
                       S2.ax32.as<uint32_t>());
    HY_CHECK_LAUNCH("mark_compact_kernel");
    S2.n = A2;
    S2.span = S1.span;
    S2.has_hb = S2.has_x32 = true;
    return HYMET_OK;
}

int marked_anchor_set(hymet_ctx *ctx, const AnchorSet &S1, const LeanJoin &lj, const uint32_t *flag, int n_q, int64_t A2,
                      AnchorSet &S2) {
    if (A2 != lj.n2) return hymet::fail(HYMET_E_INTERNAL, "hymet_mm_map: long-join anchor count mismatch");
    return compact_marked(ctx, S1, lj.mark.as<uint8_t>(), flag, n_q, A2, S2);
}

// a caller's 64-bit y values as the device holds them: the low words, and the span they share
static int narrow_y(const uint64_t *h_y, int64_t n, std::vector<uint32_t> &y32, int *span, const char *what) {
    y32.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if ((h_y[i] >> 32) != (h_y[0] >> 32)) return hymet::fail(HYMET_E_ARG, what);
        y32[(size_t)i] = (uint32_t)h_y[i];
    }
    *span = n > 0 ? (int)(h_y[0] >> 32 & 0xff) : 0;
    return HYMET_OK;
}

}  // namespace mm
}  // namespace hymet

using namespace hymet;
using namespace hymet::mm;

extern "C" int hymet_mm_chain_dp(hymet_ctx *ctx, const uint64_t *h_x, const uint64_t *h_y, int64_t n, int max_dist,
                                 int max_dist_inner, int bw, int max_chn_skip, int cap_rmq_size, float pen_gap,
                                 float pen_skip, int32_t *h_f, int64_t *h_p) {
    HY_ARG(ctx && (n == 0 || (h_x && h_y && h_f && h_p)), "hymet_mm_chain_dp: null argument");
    HY_ARG(n >= 0 && n < INT32_MAX, "hymet_mm_chain_dp: n out of range");
    if (n == 0) return HYMET_OK;
    HY_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    AnchorSet A;  // one query holding every anchor
    const int64_t h_off[2] = {0, n};
    A.n = n;
    std::vector<uint32_t> y32;  // y is 32-bit on the device: narrowed for the upload
    int rc = narrow_y(h_y, n, y32, &A.span, "hymet_mm_chain_dp: the anchors' y values carry different spans");
    if (rc) return rc;
    HY_HIP(A.ax.alloc(8 * (size_t)n, st));
    HY_HIP(A.ay.alloc(4 * (size_t)n, st));
    HY_HIP(A.d_off.alloc(sizeof h_off, st));
    HY_HIP(hipMemcpyAsync(A.ax.p, h_x, 8 * (size_t)n, hipMemcpyHostToDevice, st));
    HY_HIP(hipMemcpyAsync(A.ay.p, y32.data(), 4 * (size_t)n, hipMemcpyHostToDevice, st));
    HY_HIP(hipMemcpyAsync(A.d_off.p, h_off, sizeof h_off, hipMemcpyHostToDevice, st));
    rc = derive_heads(ctx, A);
    if (rc) return rc;
    Groups Gr;
    rc = build_groups(ctx, A, 1, Gr);
    if (rc) return rc;
    WorkList W;
    rc = build_work_list(ctx, Gr, 1, W);
    if (rc) return rc;
    DevBuf f, p;  // (the stamps are the context's, as for every caller)
    rc = chain_dp(ctx, DpArgs{max_dist, max_dist_inner, bw, max_chn_skip, cap_rmq_size, pen_gap, pen_skip, 1}, A, Gr, W, f, p);
    if (rc) return rc;
    HY_HIP(hipMemcpyAsync(h_f, f.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    std::vector<int32_t> p32((size_t)n);  // the links are 32-bit on the device: widened for the caller
    HY_HIP(hipMemcpyAsync(p32.data(), p.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HY_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; i++) h_p[i] = p32[(size_t)i];
    return HYMET_OK;
}

namespace {
__global__ __launch_bounds__(256) void stamp_nonzero_kernel(const int32_t *t, int64_t n, unsigned long long *out) {
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) c += t[i] != 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}
}  // namespace

extern "C" int hymet_mm_stamp_scratch(hymet_ctx *ctx, int64_t *capacity, int64_t *nonzero) {
    HY_ARG(ctx && capacity && nonzero, "hymet_mm_stamp_scratch: null argument");
    HY_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    HY_HIP(hipStreamSynchronize(st));
    *capacity = ctx->stamp_cap;
    *nonzero = 0;
    if (ctx->stamp_cap == 0) return HYMET_OK;
    DevBuf cnt;
    HY_HIP(cnt.alloc(8, st));
    HY_HIP(hipMemsetAsync(cnt.p, 0, 8, st));
    const int64_t nb = std::min<int64_t>(cdiv(ctx->stamp_cap, 256), (int64_t)ctx->n_cu * 8);
    hipLaunchKernelGGL(stamp_nonzero_kernel, dim3((unsigned)nb), dim3(256), 0, st, (const int32_t *)ctx->stamp, ctx->stamp_cap,
                       cnt.as<unsigned long long>());
    HY_CHECK_LAUNCH("stamp_nonzero_kernel");
    unsigned long long h = 0;
    HY_HIP(hipMemcpyAsync(&h, cnt.p, 8, hipMemcpyDeviceToHost, st));
    HY_HIP(hipStreamSynchronize(st));
    *nonzero = (int64_t)h;
    return HYMET_OK;
}

extern "C" int hymet_mm_mark_compact(hymet_ctx *ctx, const uint64_t *h_x, const uint64_t *h_y, const int32_t *h_mark, int64_t n,
                                     const int64_t *h_qoff, const uint32_t *h_qflag, int32_t n_q, uint64_t *h_ox,
                                     uint64_t *h_oy, uint32_t *h_ohb, int64_t *n_kept) {
    HY_ARG(ctx && h_x && h_y && h_mark && h_qoff && h_qflag && h_ox && h_oy && h_ohb && n_kept,
           "hymet_mm_mark_compact: null argument");
    HY_ARG(n > 0 && n < INT32_MAX && n_q > 0, "hymet_mm_mark_compact: n or n_q out of range");
    HY_ARG(h_qoff[0] == 0 && h_qoff[n_q] == n, "hymet_mm_mark_compact: query offsets do not span the anchors");
    for (int32_t q = 0; q < n_q; q++) HY_ARG(h_qoff[q] <= h_qoff[q + 1], "hymet_mm_mark_compact: query offsets not rising");
    HY_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    AnchorSet S1, S2;
    S1.n = n;
    std::vector<uint32_t> y32;
    int rc = narrow_y(h_y, n, y32, &S1.span, "hymet_mm_mark_compact: the anchors' y values carry different spans");
    if (rc) return rc;
    DevBuf mark, flag;
    HY_HIP(S1.ax.alloc(8 * (size_t)n, st));
    HY_HIP(S1.ay.alloc(4 * (size_t)n, st));
    HY_HIP(S1.d_off.alloc(8 * (size_t)(n_q + 1), st));
    // the caller's int32 marks as the device holds them: bytes, narrowed so that only 2 stays 2
    // (a stale stamp such as 258 must not truncate into a mark)
    std::vector<uint8_t> m8((size_t)n);
    for (int64_t i = 0; i < n; i++) m8[(size_t)i] = h_mark[i] == 2 ? 2 : (h_mark[i] != 0);
    HY_HIP(mark.alloc((size_t)n + 16, st));
    HY_HIP(flag.alloc(4 * (size_t)n_q, st));
    HY_HIP(hipMemcpyAsync(S1.ax.p, h_x, 8 * (size_t)n, hipMemcpyHostToDevice, st));
    HY_HIP(hipMemcpyAsync(S1.ay.p, y32.data(), 4 * (size_t)n, hipMemcpyHostToDevice, st));
    HY_HIP(hipMemcpyAsync(S1.d_off.p, h_qoff, 8 * (size_t)(n_q + 1), hipMemcpyHostToDevice, st));
    HY_HIP(hipMemcpyAsync(mark.p, m8.data(), (size_t)n, hipMemcpyHostToDevice, st));
    HY_HIP(hipMemcpyAsync(flag.p, h_qflag, 4 * (size_t)n_q, hipMemcpyHostToDevice, st));
    rc = compact_marked(ctx, S1, mark.as<uint8_t>(), flag.as<uint32_t>(), n_q, -1, S2);
    if (rc) {
        HY_HIP(hipStreamSynchronize(st));  // the uploads read the caller's arrays
        return rc;
    }
    const int64_t m = S2.n;
    std::vector<uint32_t> oy32((size_t)m);
    if (m > 0) {
        HY_HIP(hipMemcpyAsync(h_ox, S2.ax.p, 8 * (size_t)m, hipMemcpyDeviceToHost, st));
        HY_HIP(hipMemcpyAsync(oy32.data(), S2.ay.p, 4 * (size_t)m, hipMemcpyDeviceToHost, st));
        HY_HIP(hipMemcpyAsync(h_ohb, S2.hb.p, 4 * (size_t)((m + 31) / 32), hipMemcpyDeviceToHost, st));
    }
    HY_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; i < m; i++) h_oy[i] = (h_y[0] >> 32) << 32 | oy32[(size_t)i];
    *n_kept = m;
    return HYMET_OK;
}

// Mash `dist` on MI355X: the (common, denom) pair of every reference sketch x query sketch of
// two sketch DBs (the interface replaced is `mash dist REF.msh QUERY.msh`), and
// the threshold filter over the dense result (`mash dist -d`).
//
// A pair.  A (reference) and B (query) are strictly ascending lists of distinct uint64 hashes,
// truncated to their first s entries.  With U_s = the s smallest values of A u B:
//   denom = min(s, |A u B|),   common = |A n B n U_s|
// (Mash's merge loop, restated in DESIGN.md §Dist).  One wave computes one pair over the merged
// sequence of the two lists (ties: A's entry first), position by position: a match is counted at
// A's entry, and the union rank of position p is p minus the matches before p.  A pass covers a
// range of merged positions [d0, d1): lane l takes ceil((d1 - d0) / 64) consecutive positions,
// finds where they start in both lists by a binary search along its diagonal (the merge path)
// and steps through them, so every lane does the same number of steps.  The first pass covers
// [0, s).  M matches in it mean the s-th union element lies at position s + M or later, so the
// next pass covers [s, s + M), and so on until a pass finds no match: then common = the matches
// so far and the range end is the position of union rank s.  Unrelated lists take one pass over
// s of their 2s entries; a range that reaches the end of both lists means |A u B| <= s.
// The lists carry their lengths: no sentinel value, 2^64 - 1 is a hash like any other.  All
// comparisons are unsigned 64-bit; no float arithmetic, no atomics.
//
// Kernels
//   dist_tiled : a 256-thread workgroup stages a tile of TQ query sketches in LDS once, then
//                streams its share of the references through one more LDS row; each of the 4
//                waves takes the tile's queries w, w + 4, ... against the staged reference.
//                HBM traffic per pair: 8 * s / TQ bytes of reference hashes + 4 bytes of result.
//   dist_global: one wave per pair, both lists read from global memory (an s whose tile does
//                not fit the LDS, or HYMET_DIST_PATH=global).
//   select_count / select_write: per row of the dense block, the references whose common
//                reaches min_common[denom], in reference order: count, hymet_scan_u32's scan,
//                write (ballot ranks inside a row: the order is the reference order).
//   dist_tiled<true> / dist_tri_global: one DB against itself, the pairs r < q only (the lower
//                triangle; hymet_mash_dist_tri).  A workgroup clips its references to those below
//                its tile's last query and a wave skips a pair with r >= q.
//   link       : the same filter over the r < q entries of a dense block, each passing pair united
//                in a union-find over the sketches (hymet_mash_link; the rules stand at uf_find);
//                labels: every sketch's root, the smallest index of its component.
//   sp_*       : the same CSR as select over the dense block, for a threshold below 1, from the
//                pairs that share a hash only (hymet_mash_dist_sparse): postings sorted by hash,
//                one key per shared hash of a pair, keys sorted, runs of cmin or more keys go to
//                the pair routine.  link_edges: the union-find over that CSR.
//   greedy / greedy_edges: one round of the greedy choice of representatives over the r < q
//                entries of a dense block or of that CSR (hymet_mash_greedy, hymet_mash_greedy_edges;
//                the rules stand at greedy_entry).
#include "mash_rank.hpp"
#include "mm_common.hpp"
#include "sort.hpp"

#include <algorithm>
#include <cstdlib>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxS = 16384;            // hymet_sketch_max_size(): common and denom fit 16 bits
constexpr int kLdsBytes = 160 * 1024;   // per CU
constexpr int kLdsHdr = 256;            // the tile's list lengths
constexpr int kDefaultTq = 4;
constexpr int kPre = 4;                 // reference entries per thread fetched one reference ahead
constexpr int kMaxTq = 32;              // kLdsHdr / 4 would hold 64

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// (common << 16 | denom) of one pair; every lane of the wave calls it and gets the result.
// PA / PB: pointer types, so that a list in LDS is read with LDS instructions.
template <typename PA, typename PB>
__device__ __forceinline__ uint32_t wave_pair(PA A, int la, PB B, int lb, int s) {
    if (la == 0 || lb == 0) return (uint32_t)min(s, la + lb);  // wave-uniform; below both lists have an entry
    const int lane = threadIdx.x & 63;
    const int tot = la + lb;
    int d0 = 0, d1 = min(s, tot), matches = 0;
    for (;;) {  // merged positions [d0, d1); every bound is wave-uniform
        const int step = (d1 - d0 + 63) >> 6;
        const int d = min(d0 + lane * step, d1), n = min(step, d1 - d);
        // the merge path at diagonal d: i entries of A and d - i of B come first
        int lo = max(0, d - lb), hi = min(d, la);
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (A[mid] <= B[d - mid - 1])
                lo = mid + 1;
            else
                hi = mid;
        }
        // n steps from there.  No branch inside a step: both lists' next entries are loaded every
        // time, at indices clamped into the lists.
        int i = lo, j = d - lo, m = 0;
        for (int t = 0; t < n; t++) {
            const uint64_t a = A[min(i, la - 1)], b = B[min(j, lb - 1)];
            const bool in_b = j < lb;
            const bool take_a = i < la && (!in_b || a <= b);
            m += take_a && in_b && a == b ? 1 : 0;
            i += take_a ? 1 : 0;
            j += take_a ? 0 : 1;
        }
        matches += wave_sum(m);
        const int next = min(s + matches, tot);
        if (next == d1) break;
        d0 = d1;
        d1 = next;
    }
    return (uint32_t)matches << 16 | (uint32_t)min(s, tot - matches);
}

// grid: n_tiles * n_chunks blocks; block b = (tile b / n_chunks, reference chunk b % n_chunks)
// TRI: references and queries are one DB and only the pairs r < q are computed and written.  The
// tiles are taken last first: a tile's work grows with its first query, and the longest blocks
// then start first and the short ones fill the tail.
template <bool TRI>
__global__ __launch_bounds__(kThreads) void dist_tiled_kernel(const uint64_t *__restrict__ rh,
                                                              const int64_t *__restrict__ roff, int64_t n_ref,
                                                              const uint64_t *__restrict__ qh,
                                                              const int64_t *__restrict__ qoff, int64_t q_begin,
                                                              int64_t q_end, int s, int tq, int64_t n_chunks,
                                                              int64_t chunk, uint32_t *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *qlen = reinterpret_cast<int *>(smem);
    uint64_t *Q = reinterpret_cast<uint64_t *>(smem + kLdsHdr);  // tq rows of s
    uint64_t *R = Q + (size_t)tq * s;                            // the staged reference
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_tiles = gridDim.x / n_chunks;
    const int64_t tile = TRI ? n_tiles - 1 - blockIdx.x / n_chunks : blockIdx.x / n_chunks, ch = blockIdx.x % n_chunks;
    const int64_t q0 = q_begin + tile * tq;
    const int nq = (int)min((int64_t)tq, q_end - q0);
    // TRI: the references below the tile's last query
    const int64_t r0 = ch * chunk, r1 = min(r0 + chunk, TRI ? min(n_ref, q0 + nq - 1) : n_ref);
    if (TRI && r0 >= r1) return;  // workgroup-uniform, before the first barrier
    for (int t = 0; t < nq; t++) {
        const int64_t b = qoff[q0 + t];
        const int len = (int)min((int64_t)s, qoff[q0 + t + 1] - b);
        for (int e = threadIdx.x; e < len; e += kThreads) Q[(size_t)t * s + e] = qh[b + e];
        if (threadIdx.x == 0) qlen[t] = len;
    }
    // The reference after the one being compared is already on its way: its first kPre * 256
    // entries (all of them for s <= 1,024) are loaded into registers before the waves start on
    // the staged one, and stored to LDS after the next barrier.
    uint64_t pf[kPre];
    int64_t nb = 0;
    int nla = 0;
    auto prefetch = [&](int64_t r) {
        nb = roff[r];
        nla = (int)min((int64_t)s, roff[r + 1] - nb);
#pragma unroll
        for (int u = 0; u < kPre; u++) {
            const int e = u * kThreads + (int)threadIdx.x;
            pf[u] = e < nla ? rh[nb + e] : 0;
        }
    };
    if (r0 < r1) prefetch(r0);
    for (int64_t r = r0; r < r1; r++) {
        const int64_t b = nb;
        const int la = nla;
        __syncthreads();  // the readers of the previous reference are done
#pragma unroll
        for (int u = 0; u < kPre; u++) {
            const int e = u * kThreads + (int)threadIdx.x;
            if (e < la) R[e] = pf[u];
        }
        for (int e = kPre * kThreads + (int)threadIdx.x; e < la; e += kThreads) R[e] = rh[b + e];
        __syncthreads();  // the reference (and, the first time, the query tile) is staged
        if (r + 1 < r1) prefetch(r + 1);
        for (int t = wave; t < nq; t += kWaves) {
            if (TRI && r >= q0 + t) continue;  // wave-uniform
            const uint32_t v = wave_pair(R, la, Q + (size_t)t * s, qlen[t], s);
            if (lane == 0) out[(size_t)(q0 - q_begin + t) * (size_t)n_ref + (size_t)r] = v;
        }
    }
}

// one wave per pair; pair p = (row p / n_ref, reference p % n_ref)
__global__ __launch_bounds__(kThreads) void dist_global_kernel(const uint64_t *__restrict__ rh,
                                                               const int64_t *__restrict__ roff, int64_t n_ref,
                                                               const uint64_t *__restrict__ qh,
                                                               const int64_t *__restrict__ qoff, int64_t q_begin,
                                                               int64_t n_pairs, int s, uint32_t *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (p >= n_pairs) return;  // wave-uniform
    const int64_t q = q_begin + p / n_ref, r = p % n_ref;
    const int64_t rb = roff[r], qb = qoff[q];
    const int la = (int)min((int64_t)s, roff[r + 1] - rb), lb = (int)min((int64_t)s, qoff[q + 1] - qb);
    const uint32_t v = wave_pair(rh + rb, la, qh + qb, lb, s);
    if ((threadIdx.x & 63) == 0) out[p] = v;
}

// PT: pointer type, so that a table staged in LDS is read with LDS instructions
template <typename PT>
__device__ __forceinline__ bool select_pass(uint32_t v, PT minc, int s) {
    const uint32_t denom = v & 0xffffu;
    return denom <= (uint32_t)s && (v >> 16) >= (uint32_t)minc[denom];
}

// one workgroup per row of the dense block
__global__ __launch_bounds__(kThreads) void select_count_kernel(const uint32_t *__restrict__ blk, int64_t n_ref,
                                                                const uint16_t *__restrict__ minc, int s,
                                                                uint32_t *__restrict__ cnt) {
    __shared__ int ws[kWaves];
    const uint32_t *row = blk + (size_t)blockIdx.x * (size_t)n_ref;
    int c = 0;
    for (int64_t r = threadIdx.x; r < n_ref; r += kThreads) c += select_pass(row[r], minc, s) ? 1 : 0;
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kWaves; w++) t += ws[w];
        cnt[blockIdx.x] = (uint32_t)t;
    }
}

__global__ __launch_bounds__(kThreads) void select_write_kernel(const uint32_t *__restrict__ blk, int64_t n_ref,
                                                                const uint16_t *__restrict__ minc, int s,
                                                                const int64_t *__restrict__ row_off, int64_t cap,
                                                                int32_t *__restrict__ out_ref,
                                                                uint32_t *__restrict__ out_val) {
    __shared__ int ws[kWaves];
    const uint32_t *row = blk + (size_t)blockIdx.x * (size_t)n_ref;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t base = row_off[blockIdx.x];
    for (int64_t r0 = 0; r0 < n_ref; r0 += kThreads) {  // workgroup-uniform trip count
        const int64_t r = r0 + threadIdx.x;
        const uint32_t v = r < n_ref ? row[r] : 0u;
        const bool keep = r < n_ref && select_pass(v, minc, s);
        const uint64_t mask = __ballot(keep);
        if (lane == 0) ws[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            before += w < wave ? ws[w] : 0;
            all += ws[w];
        }
        const int64_t pos = base + before + __popcll(mask & ((1ull << lane) - 1));
        if (keep && pos < cap) {
            out_ref[pos] = (int32_t)r;
            out_val[pos] = v;
        }
        base += all;
        __syncthreads();
    }
}

// one wave per entry of the rows x n block; the waves of the entries r >= q leave at once
__global__ __launch_bounds__(kThreads) void dist_tri_global_kernel(const uint64_t *__restrict__ h,
                                                                   const int64_t *__restrict__ off, int64_t n,
                                                                   int64_t q_begin, int64_t n_pairs, int s,
                                                                   uint32_t *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (p >= n_pairs) return;  // wave-uniform
    const int64_t q = q_begin + p / n, r = p % n;
    if (r >= q) return;  // wave-uniform
    const int64_t rb = off[r], qb = off[q];
    const int la = (int)min((int64_t)s, off[r + 1] - rb), lb = (int)min((int64_t)s, off[q + 1] - qb);
    const uint32_t v = wave_pair(h + rb, la, h + qb, lb, s);
    if ((threadIdx.x & 63) == 0) out[p] = v;
}

// ---- union-find over the sketches of one DB (hymet_mash_link, hymet_mash_labels)
// Invariant: 0 <= parent[x] <= x; a root has parent[x] == x.  The only write that makes a root a
// non-root is the CAS in uf_unite, which stores a smaller index; path shortening stores a smaller
// ancestor (atomicMin).  So parent[x] only ever falls, through members of x's component, and a
// component's root is its smallest member whatever order the atomics land in.
// Every access to parent inside a launch is a relaxed agent-scope atomic (performed past the
// XCD-private L2s, as scan.hip argues for its hand-off), but nothing rests on a load being fresh:
//   * a stale parent[x] is an earlier value of the word, hence still an ancestor of x;
//   * only the CAS decides a link: it succeeds only while hi is a root, and then lo < hi lies in
//     another component (a root is the smallest member of its own); when it fails, the value it
//     returned is hi's parent and the union goes on from there, the word is not read again;
//   * two walks that end in the same index prove one component, for good: links are never removed.
// uf_find follows only values v with 0 <= v < x, so it ends after at most x steps on any array
// contents; any other value != x stops the walk and sets the error word (reported by
// hymet_mash_labels).  The labels run in a launch of their own, after every link.
__device__ __forceinline__ int32_t uf_ld(int32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above x as far as this thread sees it; -1 after a parent outside [0, x]
__device__ __forceinline__ int32_t uf_find(int32_t *__restrict__ parent, int32_t x, int32_t *__restrict__ err) {
    int32_t p = uf_ld(parent + x);
    for (;;) {
        if (p == x) return x;
        if (p < 0 || p > x) {
            __hip_atomic_fetch_or(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return -1;
        }
        const int32_t g = uf_ld(parent + p);  // p < x
        // shorten: x's grandparent, an ancestor below its parent (a root or a bad g: nothing stored)
        if (g >= 0 && g < p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
}

__device__ __forceinline__ void uf_unite(int32_t *__restrict__ parent, int32_t a, int32_t b,
                                         int32_t *__restrict__ err) {
    a = uf_find(parent, a, err);
    b = uf_find(parent, b, err);
    while (a >= 0 && b >= 0 && a != b) {
        const int32_t hi = max(a, b), lo = min(a, b);
        int32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        // hi was linked by another thread: seen is its parent.  lo need not be a root any more;
        // the next CAS is on the larger of the two again and decides the same way.
        if (seen < 0 || seen > hi) {
            __hip_atomic_fetch_or(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        a = uf_find(parent, seen, err);
        b = lo;
    }
}

// Workgroup w takes the rows w, w + gridDim.x, ... of the block; row `row` is sketch q = q_begin +
// row and only its entries r < q are read: 16-byte loads between the row's first and last
// 16-byte boundary, single entries before and after.  The table is staged in LDS once.
__global__ __launch_bounds__(kThreads) void link_kernel(const uint32_t *__restrict__ blk, int64_t n_rows, int64_t n,
                                                        int64_t q_begin, const uint16_t *__restrict__ minc, int s,
                                                        int32_t *__restrict__ parent,
                                                        unsigned long long *__restrict__ n_links,
                                                        int32_t *__restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ unsigned long long ws[kWaves];
    uint16_t *tab = reinterpret_cast<uint16_t *>(smem);
    for (int e = threadIdx.x; e <= s; e += kThreads) tab[e] = minc[e];
    __syncthreads();
    unsigned long long c = 0;
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int32_t q = (int32_t)(q_begin + row);
        const uint32_t *p = blk + (size_t)row * (size_t)n;
        const int64_t lim = q;  // q < n
        const int64_t head = min(lim, (int64_t)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2);
        const int64_t nvec = (lim - head) >> 2;
        auto entry = [&](int64_t r, uint32_t v) {
            if (select_pass(v, tab, s)) {
                c++;
                uf_unite(parent, q, (int32_t)r, err);
            }
        };
        if ((int64_t)threadIdx.x < head) entry(threadIdx.x, p[threadIdx.x]);
        const uint4 *pv = reinterpret_cast<const uint4 *>(p + head);
        for (int64_t i = threadIdx.x; i < nvec; i += kThreads) {
            const uint4 v = pv[i];
            const int64_t r = head + 4 * i;
            entry(r, v.x);
            entry(r + 1, v.y);
            entry(r + 2, v.z);
            entry(r + 3, v.w);
        }
        const int64_t tail = head + 4 * nvec + threadIdx.x;  // fewer than 4 entries are left
        if (tail < lim) entry(tail, p[tail]);
    }
    // the passing pairs of this workgroup: one integer atomic, so the total does not depend on order
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kWaves; w++) t += ws[w];
        if (t) atomicAdd(n_links, t);
    }
}

__global__ __launch_bounds__(kThreads) void labels_kernel(int32_t *__restrict__ parent, int64_t n,
                                                          int32_t *__restrict__ label, int32_t *__restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) label[i] = uf_find(parent, (int32_t)i, err);
}

// one workgroup per row block of the CSR: row `row` is sketch q_begin + row, its entries the
// sketches it is united with (hymet_mash_link_edges)
__global__ __launch_bounds__(kThreads) void link_edges_kernel(const int64_t *__restrict__ row_off, int64_t n_rows,
                                                              int64_t q_begin, const int32_t *__restrict__ ref_idx,
                                                              int32_t *__restrict__ parent,
                                                              unsigned long long *__restrict__ n_links,
                                                              int32_t *__restrict__ err) {
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int32_t q = (int32_t)(q_begin + row);
        const int64_t e1 = row_off[row + 1];
        for (int64_t e = row_off[row] + threadIdx.x; e < e1; e += kThreads) {
            const int32_t r = ref_idx[e];
            if (r < 0)
                __hip_atomic_fetch_or(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                uf_unite(parent, q, r, err);
        }
    }
    // the entry count is the CSR's span: one integer atomic per call
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t t = row_off[n_rows] - row_off[0];
        if (t > 0) atomicAdd(n_links, (unsigned long long)t);
    }
}

// ---- greedy representatives (hymet_mash_greedy, hymet_mash_greedy_edges; DESIGN.md §3 "Greedy derep")
// The sketches are numbered in priority order.  Walking them in that order, a sketch is a
// representative iff no earlier representative passes with it, else a member of the nearest of
// those (mash_rank.hpp's key with the representative's index as the position: equal rationals go
// to the earlier one).  That is the lexicographically first maximal independent set, reached here
// as a fixed point over rounds, one launch each.  rep[x] is the state word of sketch x:
//   kGrOpen     undecided
//   kGrPending  a member whose representative is not chosen yet: a representative passes with it,
//               and another passing neighbour is still undecided.  For every other row a
//               non-representative for good.
//   x           a representative            r != x, r >= 0   a member of representative r
// A round scans the passing entries r < q of every row q that is open or pending and reads
// rep[r] once per entry: the row sees a representative (rep[r] == r), an open neighbour, or a
// non-representative.  Seeing an open neighbour it waits (pending once it has also seen a
// representative); seeing none, it is final: its own index without a representative among its
// neighbours, else the nearest of them, all of which it has seen.
// Every access to rep inside a launch is a whole-word relaxed agent-scope atomic, as uf_ld's, and
// as there no fence protocol is needed, because nothing rests on a load being fresh: a word only
// moves open -> pending -> member or open -> final, "is a representative" and "is not one" are
// both final once seen, and the one stale value there is, open (or pending, which decides like a
// member), only makes the reader wait for the next launch, whose boundary makes every store
// visible.  Nothing spins.  rep[q] is written by the workgroup (wave) that owns row q only.
// The lowest open row of a range has no open neighbour, so every round decides one row at least,
// and the round after the last open row is gone settles the pending ones: at most n_rows + 1.
constexpr int32_t kGrOpen = -1, kGrPending = -2;
constexpr uint32_t kGrSawRep = 1, kGrSawOpen = 2;

__device__ __forceinline__ uint64_t gr_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// one passing entry (r, v) of an open or pending row; r lies in [0, q)
__device__ __forceinline__ void greedy_entry(int32_t *__restrict__ rep, int32_t r, uint32_t v, int64_t q_begin,
                                             uint64_t &best, uint32_t &flags, int32_t *__restrict__ err) {
    const int32_t sr = uf_ld(rep + r);
    if (sr == r) {
        const uint32_t d = v & 0xffffu;
        flags |= kGrSawRep;
        best = gr_min(best, hymet::mash_rank_key(min(v >> 16, d), d, (uint32_t)r));  // common > denom ranks as 1
    } else if (sr == kGrOpen) {
        flags |= kGrSawOpen;
        // a row before this call's range that no earlier call decided: the caller's error
        if (r < q_begin) __hip_atomic_fetch_or(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the state of row q after a round that saw `flags` and the nearest representative `best`
__device__ __forceinline__ int32_t greedy_decide(int32_t q, uint64_t best, uint32_t flags) {
    if (flags & kGrSawOpen) return flags & kGrSawRep ? kGrPending : kGrOpen;
    return flags & kGrSawRep ? (int32_t)(uint32_t)best : q;
}

// One round over a dense block, in link_kernel's shape: workgroup w takes the rows w, w +
// gridDim.x, ...; a decided row leaves at once.  count != 0 (a call's first round): every row
// is scanned and its passing entries are counted into *n_links.  *left: the rows still open or
// pending after the round.
__global__ __launch_bounds__(kThreads) void greedy_kernel(const uint32_t *__restrict__ blk, int64_t n_rows, int64_t n,
                                                          int64_t q_begin, const uint16_t *__restrict__ minc, int s,
                                                          int count, int32_t *__restrict__ rep,
                                                          unsigned long long *__restrict__ n_links,
                                                          int32_t *__restrict__ left, int32_t *__restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ unsigned long long ws[kWaves], ws_best[kWaves];
    __shared__ uint32_t ws_flags[kWaves];
    __shared__ int32_t s_state;
    uint16_t *tab = reinterpret_cast<uint16_t *>(smem);
    for (int e = threadIdx.x; e <= s; e += kThreads) tab[e] = minc[e];
    unsigned long long c = 0;
    int32_t n_left = 0;  // thread 0's
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int32_t q = (int32_t)(q_begin + row);
        if (threadIdx.x == 0) s_state = uf_ld(rep + q);
        __syncthreads();  // also: the table is staged
        const int32_t st = s_state;
        if (st < 0 || count) {  // workgroup-uniform
            const bool open = st < 0;
            const uint32_t *p = blk + (size_t)row * (size_t)n;
            const int64_t lim = q;  // q < n
            const int64_t head = min(lim, (int64_t)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2);
            const int64_t nvec = (lim - head) >> 2;
            uint64_t best = ~0ull;
            uint32_t flags = 0;
            auto entry = [&](int64_t r, uint32_t v) {
                if (select_pass(v, tab, s)) {
                    c += count ? 1 : 0;
                    if (open) greedy_entry(rep, (int32_t)r, v, q_begin, best, flags, err);
                }
            };
            if ((int64_t)threadIdx.x < head) entry(threadIdx.x, p[threadIdx.x]);
            const uint4 *pv = reinterpret_cast<const uint4 *>(p + head);
            for (int64_t i = threadIdx.x; i < nvec; i += kThreads) {
                const uint4 v = pv[i];
                const int64_t r = head + 4 * i;
                entry(r, v.x);
                entry(r + 1, v.y);
                entry(r + 2, v.z);
                entry(r + 3, v.w);
            }
            const int64_t tail = head + 4 * nvec + threadIdx.x;  // fewer than 4 entries are left
            if (tail < lim) entry(tail, p[tail]);
            if (open) {  // workgroup-uniform
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    best = gr_min(best, __shfl_xor((unsigned long long)best, d, 64));
                    flags |= __shfl_xor(flags, d, 64);
                }
                if ((threadIdx.x & 63) == 0) {
                    ws_best[threadIdx.x >> 6] = best;
                    ws_flags[threadIdx.x >> 6] = flags;
                }
                __syncthreads();
                if (threadIdx.x == 0) {
                    for (int w = 1; w < kWaves; w++) {
                        best = gr_min(best, ws_best[w]);
                        flags |= ws_flags[w];
                    }
                    const int32_t now = greedy_decide(q, best, flags);
                    if (now != st) __hip_atomic_store(rep + q, now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    n_left += now < 0 ? 1 : 0;
                }
            }
        }
        __syncthreads();  // s_state and the waves' words are read
    }
    if (threadIdx.x == 0 && n_left) atomicAdd(left, n_left);
    if (!count) return;  // workgroup-uniform
    // the passing pairs of this workgroup: one integer atomic, so the total does not depend on order
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kWaves; w++) t += ws[w];
        if (t) atomicAdd(n_links, t);
    }
}

// One round over a CSR whose rows are short: one wave per row, wave w of the grid takes the rows
// w, w + the grid's waves, ...  Every entry is a passing pair; one outside [0, q) sets the error
// word and is not followed.
__global__ __launch_bounds__(kThreads) void greedy_edges_kernel(const int64_t *__restrict__ row_off, int64_t n_rows,
                                                                int64_t q_begin, const int32_t *__restrict__ ref_idx,
                                                                const uint32_t *__restrict__ val, int count,
                                                                int32_t *__restrict__ rep,
                                                                unsigned long long *__restrict__ n_links,
                                                                int32_t *__restrict__ left, int32_t *__restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * kWaves;
    int32_t n_left = 0;  // lane 0's
    for (int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); row < n_rows; row += n_waves) {  // wave-uniform
        const int32_t q = (int32_t)(q_begin + row);
        const int32_t st = __shfl(lane == 0 ? uf_ld(rep + q) : 0, 0, 64);
        if (st >= 0) continue;  // wave-uniform
        const int64_t e1 = row_off[row + 1];
        uint64_t best = ~0ull;
        uint32_t flags = 0;
        for (int64_t e = row_off[row] + lane; e < e1; e += 64) {
            const int32_t r = ref_idx[e];
            if (r < 0 || r >= q)
                __hip_atomic_fetch_or(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                greedy_entry(rep, r, val[e], q_begin, best, flags, err);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            best = gr_min(best, __shfl_xor((unsigned long long)best, d, 64));
            flags |= __shfl_xor(flags, d, 64);
        }
        if (lane == 0) {
            const int32_t now = greedy_decide(q, best, flags);
            if (now != st) __hip_atomic_store(rep + q, now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            n_left += now < 0 ? 1 : 0;
        }
    }
    if (lane == 0 && n_left) atomicAdd(left, n_left);
    // the entry count is the CSR's span: one integer atomic per call
    if (count && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t t = row_off[n_rows] - row_off[0];
        if (t > 0) atomicAdd(n_links, (unsigned long long)t);
    }
}

// ---- sparse dist (hymet_mash_dist_sparse; DESIGN.md §3 "Sparse dist")
// A posting is (hash, id): ids are the references first, then the queries of the row range
// (SpSide::first_q = n_ref); in tri mode the sketches [0, q_end) once each, a sketch being a
// query when its id lies in the row range (first_q = q_begin).  After the stable sort by hash a
// run of equal hashes holds ascending ids, so the partners of a query-side posting at i --
// the reference postings of its run, or every earlier posting in tri mode -- are the cnt[i]
// postings from the run's start on.

// one workgroup per id writes the first min(len, s) hashes of its sketch
__global__ __launch_bounds__(kThreads) void sp_postings_kernel(const uint64_t *__restrict__ rh,
                                                               const int64_t *__restrict__ roff, int64_t n_side_ref,
                                                               const uint64_t *__restrict__ qh,
                                                               const int64_t *__restrict__ qoff, int64_t q_begin,
                                                               const int64_t *__restrict__ poff, int s,
                                                               uint64_t *__restrict__ key, uint32_t *__restrict__ id) {
    const int64_t i = blockIdx.x;
    const bool is_ref = i < n_side_ref;  // workgroup-uniform
    const uint64_t *h = is_ref ? rh : qh;
    const int64_t *off = is_ref ? roff : qoff;
    const int64_t k = is_ref ? i : q_begin + (i - n_side_ref);
    const int64_t b = off[k], p = poff[i];
    const int len = (int)min((int64_t)s, off[k + 1] - b);
    for (int e = threadIdx.x; e < len; e += kThreads) {
        key[p + e] = h[b + e];
        id[p + e] = (uint32_t)i;
    }
}

// mark[i] = i at the start of a run of equal hashes, else 0: its running maximum is the run start
__global__ __launch_bounds__(kThreads) void sp_mark_kernel(const uint64_t *__restrict__ key, int64_t n,
                                                           int32_t *__restrict__ mark) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) mark[i] = i > 0 && key[i] == key[i - 1] ? 0 : (int32_t)i;
}

// keys owed by every posting (cnt has n + 1 entries, the last 0 for the scan's total)
template <bool TRI>
__global__ __launch_bounds__(kThreads) void sp_count_kernel(const uint32_t *__restrict__ id,
                                                            const int32_t *__restrict__ run_start, int64_t n,
                                                            uint32_t first_q, uint32_t *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i > n) return;
    uint32_t c = 0;
    if (i < n && id[i] >= first_q) {
        const int32_t r0 = run_start[i];
        if (TRI) {
            c = (uint32_t)((int32_t)i - r0);
        } else {  // the run's reference postings come first: the first query-side one in [r0, i)
            int32_t lo = r0, hi = (int32_t)i;
            while (lo < hi) {
                const int32_t mid = lo + ((hi - lo) >> 1);
                if (id[mid] < first_q)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            c = (uint32_t)(lo - r0);
        }
    }
    cnt[i] = c;
}

// One workgroup per 256 consecutive postings: their key offsets, run starts and rows are staged
// in LDS, then the 256 lanes sweep the workgroup's keys (contiguous in the output, and in the id
// array inside one posting's share), finding each key's posting by binary search in LDS -- as
// write_anchor_keys_kernel does, since one run can hold thousands of postings.
__global__ __launch_bounds__(kThreads) void sp_emit_kernel(const uint32_t *__restrict__ id,
                                                           const int32_t *__restrict__ run_start,
                                                           const int64_t *__restrict__ eoff, int64_t n, uint32_t first_q,
                                                           int rb, uint64_t *__restrict__ key) {
    __shared__ int64_t s_a[kThreads + 1];
    __shared__ int32_t s_r[kThreads];
    __shared__ uint32_t s_q[kThreads];
    const int tid = threadIdx.x;
    const int64_t m0 = (int64_t)blockIdx.x * kThreads;
    const int cnt = (int)min((int64_t)kThreads, n - m0);
    if (tid < cnt) {
        s_a[tid] = eoff[m0 + tid];
        s_r[tid] = run_start[m0 + tid];
        s_q[tid] = id[m0 + tid] - first_q;  // only read for a query-side posting
    }
    if (tid == 0) s_a[cnt] = eoff[m0 + cnt];
    __syncthreads();
    const int64_t a0 = s_a[0], a1 = s_a[cnt];
    for (int64_t a = a0 + tid; a < a1; a += kThreads) {
        int lo = 0, hi = cnt - 1;  // last posting with s_a <= a (its share is non-empty)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_a[mid] <= a)
                lo = mid;
            else
                hi = mid - 1;
        }
        const uint32_t r = id[(int64_t)s_r[lo] + (a - s_a[lo])];
        key[a] = (uint64_t)s_q[lo] << rb | r;
    }
}

// The pairs of two empty sketches, which no posting finds: empty query j (row eq_row[j]) pairs
// with the first epre[j + 1] - epre[j] empty references er[]; key e belongs to the last j with
// epre[j] <= e.
__global__ __launch_bounds__(kThreads) void sp_empty_keys_kernel(const uint32_t *__restrict__ eq_row,
                                                                 const int64_t *__restrict__ epre, int64_t n_eq,
                                                                 const uint32_t *__restrict__ er, int64_t n_keys, int rb,
                                                                 uint64_t *__restrict__ key) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n_keys) return;
    int64_t lo = 0, hi = n_eq - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (epre[mid] <= e)
            lo = mid;
        else
            hi = mid - 1;
    }
    key[e] = (uint64_t)eq_row[lo] << rb | er[e - epre[lo]];
}

// keep[i] = 1 at the first key of a run that is a candidate: cmin or more equal keys (sorted, so
// the key cmin - 1 places on decides), or a pair of two empty sketches (a run of one; looked up
// only when the call added such keys).  keep has n + 1 entries, the last 0.
__global__ __launch_bounds__(kThreads) void sp_runs_kernel(const uint64_t *__restrict__ key, int64_t n, int cmin, int rb,
                                                           const int64_t *__restrict__ roff,
                                                           const int64_t *__restrict__ qoff, int64_t q_begin,
                                                           int has_empty, uint32_t *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i > n) return;
    bool kp = false;
    if (i < n) {
        const uint64_t k = key[i];
        if (i == 0 || key[i - 1] != k) {
            kp = i + cmin - 1 < n && key[i + cmin - 1] == k;
            if (!kp && has_empty) {
                const int64_t r = (int64_t)(k & ((1ull << rb) - 1)), q = q_begin + (int64_t)(k >> rb);
                kp = roff[r + 1] == roff[r] && qoff[q + 1] == qoff[q];
            }
        }
    }
    keep[i] = kp ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void sp_compact_kernel(const uint64_t *__restrict__ key,
                                                              const uint32_t *__restrict__ keep,
                                                              const int64_t *__restrict__ pos, int64_t n,
                                                              uint64_t *__restrict__ cand) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n && keep[i]) cand[pos[i]] = key[i];
}

// one wave per candidate: the pair routine on the two lists in global memory, and the filter
// (pass has n_cand + 1 entries, the last zeroed by the host)
__global__ __launch_bounds__(kThreads) void sp_exact_kernel(const uint64_t *__restrict__ rh,
                                                            const int64_t *__restrict__ roff,
                                                            const uint64_t *__restrict__ qh,
                                                            const int64_t *__restrict__ qoff, int64_t q_begin,
                                                            const uint64_t *__restrict__ cand, int64_t n_cand, int rb,
                                                            int s, const uint16_t *__restrict__ minc,
                                                            uint32_t *__restrict__ val, uint32_t *__restrict__ pass) {
    const int64_t c = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (c >= n_cand) return;  // wave-uniform
    const uint64_t k = cand[c];
    const int64_t r = (int64_t)(k & ((1ull << rb) - 1)), q = q_begin + (int64_t)(k >> rb);
    const int64_t b0 = roff[r], b1 = qoff[q];
    const int la = (int)min((int64_t)s, roff[r + 1] - b0), lb = (int)min((int64_t)s, qoff[q + 1] - b1);
    const uint32_t v = wave_pair(rh + b0, la, qh + b1, lb, s);
    if ((threadIdx.x & 63) == 0) {
        val[c] = v;
        pass[c] = select_pass(v, minc, s) ? 1u : 0u;
    }
}

// row_off[row], row in [0, rows]: the passing entries before the row's first candidate (the
// candidates are in (row, reference) order; ppos has n_cand + 1 entries)
__global__ __launch_bounds__(kThreads) void sp_row_off_kernel(const uint64_t *__restrict__ cand, int64_t n_cand, int rb,
                                                              const int64_t *__restrict__ ppos, int64_t rows,
                                                              int64_t *__restrict__ row_off) {
    const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (row > rows) return;
    const uint64_t first = (uint64_t)row << rb;
    int64_t lo = 0, hi = n_cand;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cand[mid] < first)
            lo = mid + 1;
        else
            hi = mid;
    }
    row_off[row] = ppos[lo];
}

__global__ __launch_bounds__(kThreads) void sp_write_kernel(const uint64_t *__restrict__ cand,
                                                            const uint32_t *__restrict__ val,
                                                            const uint32_t *__restrict__ pass,
                                                            const int64_t *__restrict__ ppos, int64_t n_cand, int rb,
                                                            int32_t *__restrict__ out_ref, uint32_t *__restrict__ out_val) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= n_cand || !pass[c]) return;
    const int64_t p = ppos[c];  // below the total, which the host checked against the capacity
    out_ref[p] = (int32_t)(cand[c] & ((1ull << rb) - 1));
    out_val[p] = val[c];
}

// path 0: tiled where the tile fits, 1: always the plain kernel; tq 0: the default tile
struct DistCfg {
    int path = 0, tq = 0;
};
DistCfg &cfg() {
    static DistCfg c = [] {  // a process-wide setting (hymet_mash_dist_tune): the environment gives its initial value
        DistCfg d;
        const char *p = hymet::env_str("HYMET_DIST_PATH");
        if (p && std::string(p) == "global") d.path = 1;
        d.tq = (int)hymet::env_int("HYMET_DIST_TQ", d.tq, 0, kMaxTq);
        return d;
    }();
    return c;
}

// query sketches per tile for sketch size s; 0: the plain path
int tile_for(int s) {
    const DistCfg &c = cfg();
    if (c.path == 1 || s < 1 || s > kMaxS) return 0;
    const int fit = (kLdsBytes - kLdsHdr) / (8 * s) - 1;  // rows beside the reference's
    const int tq = std::min(c.tq > 0 ? c.tq : kDefaultTq, fit);
    return tq >= 2 ? tq : 0;
}

// offsets [0, n] of a device CSR: non-decreasing, inside [0, n_hashes]; keep: the host copy
int check_offsets(hymet_ctx *ctx, const int64_t *d_off, int64_t n, int64_t n_hashes, const char *what,
                  std::vector<int64_t> *keep = nullptr) {
    std::vector<int64_t> mine;
    std::vector<int64_t> &off = keep ? *keep : mine;
    off.resize((size_t)n + 1);
    HY_HIP(hipMemcpyAsync(off.data(), d_off, 8 * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream));
    HY_HIP(hipStreamSynchronize(ctx->stream));
    HY_ARG(off[0] >= 0, std::string("hymet_mash_dist: ") + what + " offsets start below 0");
    for (int64_t i = 0; i < n; i++)
        HY_ARG(off[i] <= off[i + 1],
               std::string("hymet_mash_dist: ") + what + " offset " + std::to_string(i + 1) + " decreases");
    HY_ARG(off[n] <= n_hashes, std::string("hymet_mash_dist: ") + what + " offsets run past the hash array");
    return HYMET_OK;
}

// rounds queued between two reads of the undecided count (HYMET_GREEDY_BATCH; DESIGN.md §3
// "Greedy derep"): a round over a decided range only reads its state words
constexpr int kGreedyBatch = 4, kGreedyMaxBatch = 16;

// The rounds of one greedy call over n_rows rows: round(count, d_left) queues one launch that
// adds the rows it leaves undecided to *d_left.  Ends with the first round that leaves none, and
// after n_rows + 1 rounds at the latest (then with an error: greedy_entry's argument bounds them).
template <typename Round>
int greedy_rounds(hymet_ctx *ctx, const char *what, int64_t n_rows, int32_t *rounds, Round round) {
    hipStream_t st = ctx->stream;
    const int batch = (int)hymet::env_int("HYMET_GREEDY_BATCH", kGreedyBatch, 1, kGreedyMaxBatch);
    int32_t *err = ctx->dctr + hymet::mm::kCtrGreedyErr;
    hymet::mm::DevBuf left;
    HY_HIP(left.alloc(4 * kGreedyMaxBatch, st));
    const int64_t bound = n_rows + 1;
    int64_t done = 0;
    while (done < bound) {
        const int nb = (int)std::min<int64_t>(batch, bound - done);
        HY_HIP(hipMemsetAsync(left.p, 0, 4 * kGreedyMaxBatch, st));
        for (int b = 0; b < nb; b++) {
            const int rc = round(done + b == 0 ? 1 : 0, left.as<int32_t>() + b);
            if (rc) return rc;
        }
        int32_t h_left[kGreedyMaxBatch], bad = 0;
        HY_HIP(hipMemcpyAsync(h_left, left.p, 4 * (size_t)nb, hipMemcpyDeviceToHost, st));
        HY_HIP(hipMemcpyAsync(&bad, err, 4, hipMemcpyDeviceToHost, st));
        HY_HIP(hipStreamSynchronize(st));
        if (bad) {
            *rounds = (int32_t)std::min<int64_t>(done + nb, 0x7fffffff);
            HY_HIP(hipMemsetAsync(err, 0, 4, st));  // left zeroed for the next call
            return hymet::fail(HYMET_E_ARG, std::string(what) + ": a passing row before the range is undecided, or a CSR "
                                                                "index lies outside [0, q)");
        }
        for (int b = 0; b < nb; b++) {
            done++;
            if (h_left[b] == 0) {
                *rounds = (int32_t)std::min<int64_t>(done, 0x7fffffff);
                return HYMET_OK;
            }
        }
    }
    *rounds = (int32_t)std::min<int64_t>(done, 0x7fffffff);
    return hymet::fail(HYMET_E_INTERNAL, std::string(what) + ": rows left undecided after n_rows + 1 rounds");
}

}  // namespace

extern "C" {

int hymet_mash_dist_tile(int32_t s) { return tile_for(s); }

int hymet_mash_dist_tune(int path, int tq) {
    HY_ARG(path >= -1 && path <= 1 && tq >= -1 && tq <= kMaxTq, "hymet_mash_dist_tune: path in -1..1, tq in -1.." +
                                                                     std::to_string(kMaxTq));
    if (path >= 0) cfg().path = path;
    if (tq >= 0) cfg().tq = tq;
    return HYMET_OK;
}

int hymet_mash_dist(hymet_ctx *ctx, const uint64_t *d_ref_hashes, int64_t n_ref_hashes, const int64_t *d_ref_off,
                    int64_t n_ref, const uint64_t *d_qry_hashes, int64_t n_qry_hashes, const int64_t *d_qry_off,
                    int64_t n_qry, int64_t q_begin, int64_t q_end, int32_t s, uint32_t *d_out) {
    HY_ARG(ctx, "hymet_mash_dist: null context");
    HY_ARG(s >= 1 && s <= kMaxS, "hymet_mash_dist: sketch size must be in 1.." + std::to_string(kMaxS));
    HY_ARG(n_ref >= 0 && n_qry >= 0 && n_ref_hashes >= 0 && n_qry_hashes >= 0, "hymet_mash_dist: negative count");
    HY_ARG(q_begin >= 0 && q_begin <= q_end && q_end <= n_qry, "hymet_mash_dist: row range outside [0, n_qry]");
    HY_ARG(d_ref_off && d_qry_off, "hymet_mash_dist: null offsets");
    HY_ARG((n_ref_hashes == 0 || d_ref_hashes) && (n_qry_hashes == 0 || d_qry_hashes), "hymet_mash_dist: null hashes");
    HY_HIP(hipSetDevice(ctx->device));
    int rc = check_offsets(ctx, d_ref_off, n_ref, n_ref_hashes, "reference");
    if (rc) return rc;
    rc = check_offsets(ctx, d_qry_off, n_qry, n_qry_hashes, "query");
    if (rc) return rc;
    const int64_t rows = q_end - q_begin;
    if (rows == 0 || n_ref == 0) return HYMET_OK;
    HY_ARG(d_out, "hymet_mash_dist: null output");
    HY_ARG(rows <= (1ll << 62) / n_ref, "hymet_mash_dist: too many pairs");
    const int64_t n_pairs = rows * n_ref;
    hipStream_t st = ctx->stream;
    const int tq = tile_for(s);
    if (tq == 0) {
        const int64_t nb = hymet::cdiv(n_pairs, kWaves);
        HY_ARG(nb < (1ll << 31), "hymet_mash_dist: more than 2^33 pairs in one call");
        hymet::ProfScope _ps(ctx, "mash_dist", (8.0 * n_ref_hashes + 4.0 * n_ref) * (double)rows);
        hipLaunchKernelGGL(dist_global_kernel, dim3((unsigned)nb), dim3(kThreads), 0, st, d_ref_hashes, d_ref_off, n_ref,
                           d_qry_hashes, d_qry_off, q_begin, n_pairs, (int)s, d_out);
        HY_CHECK_LAUNCH("dist_global_kernel");
        return HYMET_OK;
    }
    const int64_t n_tiles = hymet::cdiv(rows, tq);
    // enough workgroups to fill the card several times over, each with at least 16 references
    // behind one staging of its query tile
    int64_t n_chunks = std::max<int64_t>(1, std::min(hymet::cdiv((int64_t)ctx->n_cu * 8, n_tiles), hymet::cdiv(n_ref, 16)));
    const int64_t chunk = hymet::cdiv(n_ref, n_chunks);
    n_chunks = hymet::cdiv(n_ref, chunk);
    HY_ARG(n_tiles < (1ll << 31) / n_chunks, "hymet_mash_dist: too many tiles in one call");
    const size_t lds = (size_t)kLdsHdr + 8 * (size_t)s * (size_t)(tq + 1);
    if (lds > 64 * 1024)
        HY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&dist_tiled_kernel<false>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hymet::ProfScope _ps(ctx, "mash_dist", 8.0 * n_ref_hashes * (double)n_tiles + 4.0 * (double)n_pairs);
    hipLaunchKernelGGL(dist_tiled_kernel<false>, dim3((unsigned)(n_tiles * n_chunks)), dim3(kThreads), lds, st, d_ref_hashes,
                       d_ref_off, n_ref, d_qry_hashes, d_qry_off, q_begin, q_end, (int)s, tq, n_chunks, chunk, d_out);
    HY_CHECK_LAUNCH("dist_tiled_kernel");
    return HYMET_OK;
}

int hymet_mash_dist_tri(hymet_ctx *ctx, const uint64_t *d_hashes, int64_t n_hashes, const int64_t *d_off, int64_t n,
                        int64_t q_begin, int64_t q_end, int32_t s, uint32_t *d_out) {
    HY_ARG(ctx, "hymet_mash_dist_tri: null context");
    HY_ARG(s >= 1 && s <= kMaxS, "hymet_mash_dist_tri: sketch size must be in 1.." + std::to_string(kMaxS));
    HY_ARG(n >= 0 && n < (1ll << 31) && n_hashes >= 0, "hymet_mash_dist_tri: count out of range");
    HY_ARG(q_begin >= 0 && q_begin <= q_end && q_end <= n, "hymet_mash_dist_tri: row range outside [0, n]");
    HY_ARG(d_off, "hymet_mash_dist_tri: null offsets");
    HY_ARG(n_hashes == 0 || d_hashes, "hymet_mash_dist_tri: null hashes");
    HY_HIP(hipSetDevice(ctx->device));
    std::vector<int64_t> off;
    const int rc = check_offsets(ctx, d_off, n, n_hashes, "sketch", &off);
    if (rc) return rc;
    const int64_t rows = q_end - q_begin;
    if (rows == 0 || q_end <= 1) return HYMET_OK;  // row 0 has no earlier sketch
    HY_ARG(d_out, "hymet_mash_dist_tri: null output");
    const int64_t n_pairs = rows * n;  // below 2^62
    const double written = 0.5 * ((double)q_end * (double)(q_end - 1) - (double)q_begin * (double)(q_begin - 1));
    hipStream_t st = ctx->stream;
    const int tq = tile_for(s);
    if (tq == 0) {
        const int64_t nb = hymet::cdiv(n_pairs, kWaves);
        HY_ARG(nb < (1ll << 31), "hymet_mash_dist_tri: more than 2^33 entries in one call");
        double read = 0.0;  // both lists of every written pair
        if (ctx->prof)
            for (int64_t q = std::max<int64_t>(q_begin, 1); q < q_end; q++)
                read += 8.0 * ((double)std::min<int64_t>(s, off[q + 1] - off[q]) * (double)q);
        hymet::ProfScope _ps(ctx, "mash_dist_tri", 2.0 * read + 4.0 * written);
        hipLaunchKernelGGL(dist_tri_global_kernel, dim3((unsigned)nb), dim3(kThreads), 0, st, d_hashes, d_off, n, q_begin,
                           n_pairs, (int)s, d_out);
        HY_CHECK_LAUNCH("dist_tri_global_kernel");
        return HYMET_OK;
    }
    const int64_t n_tiles = hymet::cdiv(rows, tq);
    // the chunks are cut over the references below the call's last query, sized as hymet_mash_dist's
    const int64_t n_below = q_end - 1;
    int64_t n_chunks =
        std::max<int64_t>(1, std::min(hymet::cdiv((int64_t)ctx->n_cu * 8, n_tiles), hymet::cdiv(n_below, 16)));
    const int64_t chunk = hymet::cdiv(n_below, n_chunks);
    n_chunks = hymet::cdiv(n_below, chunk);
    HY_ARG(n_tiles < (1ll << 31) / n_chunks, "hymet_mash_dist_tri: too many tiles in one call");
    const size_t lds = (size_t)kLdsHdr + 8 * (size_t)s * (size_t)(tq + 1);
    if (lds > 64 * 1024)
        HY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&dist_tiled_kernel<true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    double staged = 0.0;  // reference hashes staged per tile, after the clip to the tile's last query
    if (ctx->prof) {
        std::vector<double> below((size_t)q_end, 0.0);  // below[x]: hashes read of the sketches [0, x)
        for (int64_t r = 0; r + 1 < q_end; r++) below[r + 1] = below[r] + (double)std::min<int64_t>(s, off[r + 1] - off[r]);
        for (int64_t t = 0; t < n_tiles; t++) staged += below[std::min(q_end, q_begin + (t + 1) * tq) - 1];
    }
    hymet::ProfScope _ps(ctx, "mash_dist_tri", 8.0 * staged + 4.0 * written);
    hipLaunchKernelGGL(dist_tiled_kernel<true>, dim3((unsigned)(n_tiles * n_chunks)), dim3(kThreads), lds, st, d_hashes,
                       d_off, n, d_hashes, d_off, q_begin, q_end, (int)s, tq, n_chunks, chunk, d_out);
    HY_CHECK_LAUNCH("dist_tiled_kernel<tri>");
    return HYMET_OK;
}

int hymet_mash_link(hymet_ctx *ctx, const uint32_t *d_block, int64_t n_rows, int64_t n, int64_t q_begin,
                    const uint16_t *d_min_common, int32_t s, int32_t *d_parent, uint64_t *d_n_links) {
    HY_ARG(ctx, "hymet_mash_link: null context");
    HY_ARG(s >= 1 && s <= kMaxS, "hymet_mash_link: sketch size must be in 1.." + std::to_string(kMaxS));
    HY_ARG(n >= 0 && n < (1ll << 31), "hymet_mash_link: n outside [0, 2^31)");
    HY_ARG(n_rows >= 0 && q_begin >= 0 && q_begin <= n && n_rows <= n - q_begin, "hymet_mash_link: rows outside [0, n]");
    HY_ARG(d_min_common && d_n_links, "hymet_mash_link: null argument");
    HY_HIP(hipSetDevice(ctx->device));
    if (n_rows == 0 || q_begin + n_rows <= 1) return HYMET_OK;
    HY_ARG(d_block && d_parent, "hymet_mash_link: null argument");
    HY_ARG((reinterpret_cast<uintptr_t>(d_block) & 3) == 0, "hymet_mash_link: block not 4-byte aligned");
    const double tri =
        0.5 * ((double)(q_begin + n_rows) * (double)(q_begin + n_rows - 1) - (double)q_begin * (double)(q_begin - 1));
    const int64_t nb = std::min<int64_t>(n_rows, (int64_t)ctx->n_cu * 8);
    hymet::ProfScope _ps(ctx, "mash_link", 4.0 * tri);
    hipLaunchKernelGGL(link_kernel, dim3((unsigned)nb), dim3(kThreads), 2 * ((size_t)s + 1), ctx->stream, d_block, n_rows, n,
                       q_begin, d_min_common, (int)s, d_parent, reinterpret_cast<unsigned long long *>(d_n_links),
                       ctx->dctr + hymet::mm::kCtrUfErr);
    HY_CHECK_LAUNCH("link_kernel");
    return HYMET_OK;
}

int hymet_mash_labels(hymet_ctx *ctx, int32_t *d_parent, int64_t n, int32_t *d_label) {
    HY_ARG(ctx, "hymet_mash_labels: null context");
    HY_ARG(n >= 0 && n < (1ll << 31), "hymet_mash_labels: n outside [0, 2^31)");
    HY_ARG(n == 0 || (d_parent && d_label), "hymet_mash_labels: null argument");
    HY_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int32_t *err = ctx->dctr + hymet::mm::kCtrUfErr;
    if (n > 0) {
        hymet::ProfScope _ps(ctx, "mash_labels", 8.0 * (double)n);
        hipLaunchKernelGGL(labels_kernel, dim3((unsigned)hymet::cdiv(n, kThreads)), dim3(kThreads), 0, st, d_parent, n,
                           d_label, err);
        HY_CHECK_LAUNCH("labels_kernel");
    }
    int32_t bad = 0;
    HY_HIP(hipMemcpyAsync(&bad, err, 4, hipMemcpyDeviceToHost, st));
    HY_HIP(hipStreamSynchronize(st));
    if (bad) {
        HY_HIP(hipMemsetAsync(err, 0, 4, st));  // left zeroed for the next clustering
        return hymet::fail(HYMET_E_ARG, "hymet_mash_labels: a parent outside [0, x] was met");
    }
    return HYMET_OK;
}

int hymet_mash_link_edges(hymet_ctx *ctx, const int64_t *d_row_off, int64_t n_rows, int64_t q_begin,
                          const int32_t *d_ref_idx, int32_t *d_parent, uint64_t *d_n_links) {
    HY_ARG(ctx, "hymet_mash_link_edges: null context");
    HY_ARG(n_rows >= 0 && q_begin >= 0 && q_begin < (1ll << 31) && n_rows < (1ll << 31) - q_begin,
           "hymet_mash_link_edges: rows outside [0, 2^31)");
    HY_ARG(d_n_links, "hymet_mash_link_edges: null argument");
    HY_HIP(hipSetDevice(ctx->device));
    if (n_rows == 0) return HYMET_OK;
    HY_ARG(d_row_off && d_ref_idx && d_parent, "hymet_mash_link_edges: null argument");
    const int64_t nb = std::min<int64_t>(n_rows, (int64_t)ctx->n_cu * 8);
    hymet::ProfScope _ps(ctx, "mash_link_edges", 8.0 * (double)n_rows);
    hipLaunchKernelGGL(link_edges_kernel, dim3((unsigned)nb), dim3(kThreads), 0, ctx->stream, d_row_off, n_rows, q_begin,
                       d_ref_idx, d_parent, reinterpret_cast<unsigned long long *>(d_n_links),
                       ctx->dctr + hymet::mm::kCtrUfErr);
    HY_CHECK_LAUNCH("link_edges_kernel");
    return HYMET_OK;
}

int hymet_mash_greedy(hymet_ctx *ctx, const uint32_t *d_block, int64_t n_rows, int64_t n, int64_t q_begin,
                      const uint16_t *d_min_common, int32_t s, int32_t *d_rep, uint64_t *d_n_links, int32_t *rounds) {
    HY_ARG(ctx && rounds, "hymet_mash_greedy: null argument");
    *rounds = 0;
    HY_ARG(s >= 1 && s <= kMaxS, "hymet_mash_greedy: sketch size must be in 1.." + std::to_string(kMaxS));
    HY_ARG(n >= 0 && n < (1ll << 31), "hymet_mash_greedy: n outside [0, 2^31)");
    HY_ARG(n_rows >= 0 && q_begin >= 0 && q_begin <= n && n_rows <= n - q_begin, "hymet_mash_greedy: rows outside [0, n]");
    HY_ARG(d_min_common && d_n_links, "hymet_mash_greedy: null argument");
    HY_HIP(hipSetDevice(ctx->device));
    if (n_rows == 0) return HYMET_OK;
    HY_ARG(d_block && d_rep, "hymet_mash_greedy: null argument");
    HY_ARG((reinterpret_cast<uintptr_t>(d_block) & 3) == 0, "hymet_mash_greedy: block not 4-byte aligned");
    const double tri =
        0.5 * ((double)(q_begin + n_rows) * (double)(q_begin + n_rows - 1) - (double)q_begin * (double)(q_begin - 1));
    const int64_t nb = std::min<int64_t>(n_rows, (int64_t)ctx->n_cu * 8);
    hymet::ProfScope _ps(ctx, "mash_greedy", 4.0 * tri);  // the first round's; a later one reads its open rows
    return greedy_rounds(ctx, "hymet_mash_greedy", n_rows, rounds, [&](int count, int32_t *d_left) -> int {
        hipLaunchKernelGGL(greedy_kernel, dim3((unsigned)nb), dim3(kThreads), 2 * ((size_t)s + 1), ctx->stream, d_block, n_rows,
                           n, q_begin, d_min_common, (int)s, count, d_rep, reinterpret_cast<unsigned long long *>(d_n_links),
                           d_left, ctx->dctr + hymet::mm::kCtrGreedyErr);
        HY_CHECK_LAUNCH("greedy_kernel");
        return HYMET_OK;
    });
}

int hymet_mash_greedy_edges(hymet_ctx *ctx, const int64_t *d_row_off, int64_t n_rows, int64_t q_begin,
                            const int32_t *d_ref_idx, const uint32_t *d_val, int32_t s, int32_t *d_rep,
                            uint64_t *d_n_links, int32_t *rounds) {
    HY_ARG(ctx && rounds, "hymet_mash_greedy_edges: null argument");
    *rounds = 0;
    HY_ARG(s >= 1 && s <= kMaxS, "hymet_mash_greedy_edges: sketch size must be in 1.." + std::to_string(kMaxS));
    HY_ARG(n_rows >= 0 && q_begin >= 0 && q_begin < (1ll << 31) && n_rows < (1ll << 31) - q_begin,
           "hymet_mash_greedy_edges: rows outside [0, 2^31)");
    HY_ARG(d_n_links, "hymet_mash_greedy_edges: null argument");
    HY_HIP(hipSetDevice(ctx->device));
    if (n_rows == 0) return HYMET_OK;
    HY_ARG(d_row_off && d_ref_idx && d_val && d_rep, "hymet_mash_greedy_edges: null argument");
    const int64_t nb = std::min<int64_t>(hymet::cdiv(n_rows, kWaves), (int64_t)ctx->n_cu * 8);
    // the entries are not known here: two offsets and a state word per row of the first round
    hymet::ProfScope _ps(ctx, "mash_greedy_edges", 20.0 * (double)n_rows);
    return greedy_rounds(ctx, "hymet_mash_greedy_edges", n_rows, rounds, [&](int count, int32_t *d_left) -> int {
        hipLaunchKernelGGL(greedy_edges_kernel, dim3((unsigned)nb), dim3(kThreads), 0, ctx->stream, d_row_off, n_rows, q_begin,
                           d_ref_idx, d_val, count, d_rep, reinterpret_cast<unsigned long long *>(d_n_links), d_left,
                           ctx->dctr + hymet::mm::kCtrGreedyErr);
        HY_CHECK_LAUNCH("greedy_edges_kernel");
        return HYMET_OK;
    });
}

int hymet_mash_dist_sparse(hymet_ctx *ctx, const uint64_t *d_ref_hashes, int64_t n_ref_hashes, const int64_t *d_ref_off,
                           int64_t n_ref, const uint64_t *d_qry_hashes, int64_t n_qry_hashes, const int64_t *d_qry_off,
                           int64_t n_qry, int64_t q_begin, int64_t q_end, int32_t s, int tri,
                           const uint16_t *d_min_common, int32_t cmin, int64_t max_pairs, int64_t *d_row_off,
                           int32_t *d_ref_idx, uint32_t *d_val, int64_t cap, int64_t *total,
                           hymet_sparse_counters *counters) {
    using hymet::cdiv;
    using hymet::mm::DevBuf;
    HY_ARG(ctx && total && counters, "hymet_mash_dist_sparse: null argument");
    *total = 0;
    counters->postings = counters->emitted = counters->candidates = 0;
    HY_ARG(s >= 1 && s <= kMaxS, "hymet_mash_dist_sparse: sketch size must be in 1.." + std::to_string(kMaxS));
    HY_ARG(n_ref >= 0 && n_ref < (1ll << 31) && n_qry >= 0 && n_ref_hashes >= 0 && n_qry_hashes >= 0,
           "hymet_mash_dist_sparse: count out of range");
    HY_ARG(q_begin >= 0 && q_begin <= q_end && q_end <= n_qry, "hymet_mash_dist_sparse: row range outside [0, n_qry]");
    HY_ARG(q_end - q_begin < (1ll << 31) - 1, "hymet_mash_dist_sparse: more than 2^31 rows in one call");
    HY_ARG(d_ref_off && d_qry_off, "hymet_mash_dist_sparse: null offsets");
    HY_ARG((n_ref_hashes == 0 || d_ref_hashes) && (n_qry_hashes == 0 || d_qry_hashes),
           "hymet_mash_dist_sparse: null hashes");
    HY_ARG(!tri || (d_qry_hashes == d_ref_hashes && d_qry_off == d_ref_off && n_qry == n_ref && n_qry_hashes == n_ref_hashes),
           "hymet_mash_dist_sparse: tri mode takes one DB as both arguments");
    HY_ARG(d_row_off && d_min_common, "hymet_mash_dist_sparse: null argument");
    HY_ARG(cmin >= 1 && max_pairs >= 0 && cap >= 0, "hymet_mash_dist_sparse: cmin below 1 or a negative bound");
    HY_HIP(hipSetDevice(ctx->device));
    std::vector<int64_t> roff, qoff_own;
    int rc = check_offsets(ctx, d_ref_off, n_ref, n_ref_hashes, tri ? "sketch" : "reference", &roff);
    if (rc) return rc;
    if (!tri) {
        rc = check_offsets(ctx, d_qry_off, n_qry, n_qry_hashes, "query", &qoff_own);
        if (rc) return rc;
    }
    const std::vector<int64_t> &qoff = tri ? roff : qoff_own;
    hipStream_t st = ctx->stream;
    const int64_t rows = q_end - q_begin;
    auto no_entries = [&]() -> int {
        HY_HIP(hipMemsetAsync(d_row_off, 0, 8 * (size_t)(rows + 1), st));
        HY_HIP(hipStreamSynchronize(st));
        return HYMET_OK;
    };
    if (rows == 0 || n_ref == 0) return no_entries();
    const int rb = hymet::mm::bits_for(n_ref), kb = rb + hymet::mm::bits_for(rows - 1);  // at most 31 + 31

    // ids and the posting offset of each, from the offsets the check copied
    const int64_t n_side_ref = tri ? q_end : n_ref, n_ids = tri ? q_end : n_ref + rows;
    const uint32_t first_q = (uint32_t)(tri ? q_begin : n_ref);
    HY_ARG(n_ids < (1ll << 31), "hymet_mash_dist_sparse: more than 2^31 sketches in one call");
    std::vector<int64_t> poff((size_t)n_ids + 1, 0);
    for (int64_t i = 0; i < n_ids; i++) {
        const int64_t len = i < n_side_ref ? roff[i + 1] - roff[i]
                                           : qoff[q_begin + (i - n_side_ref) + 1] - qoff[q_begin + (i - n_side_ref)];
        poff[i + 1] = poff[i] + std::min<int64_t>(s, len);
    }
    const int64_t P = poff[n_ids];
    HY_ARG(P < (1ll << 31), "hymet_mash_dist_sparse: more than 2^31 postings in one call: split the row range");
    counters->postings = P;
    // the pairs of two empty sketches: empty query j with the empty references before epre's step
    std::vector<uint32_t> er, eq_row;
    std::vector<int64_t> epre(1, 0);
    for (int64_t r = 0; r < n_side_ref; r++)
        if (roff[r + 1] == roff[r]) er.push_back((uint32_t)r);
    {
        size_t below = 0;  // tri: the empty sketches before q
        for (int64_t q = q_begin; q < q_end && !er.empty(); q++) {
            if (qoff[q + 1] != qoff[q]) continue;
            while (tri && below < er.size() && (int64_t)er[below] < q) below++;
            const int64_t k = tri ? (int64_t)below : (int64_t)er.size();
            if (k == 0) continue;
            eq_row.push_back((uint32_t)(q - q_begin));
            epre.push_back(epre.back() + k);
        }
    }
    const int64_t n_empty = epre.back();

    int64_t emitted = 0;
    DevBuf key0, key1;  // the pair keys and the sort's second buffer
    {
        // what the emit reads of the postings; released before the keys are sorted
        DevBuf d_poff, pk0, pk1, pv0, pv1, mark, run_start, eoff, mpart;
        uint32_t *ids = nullptr;
        if (P > 0) {
            HY_HIP(d_poff.alloc(8 * (size_t)(n_ids + 1), st));
            HY_HIP(pk0.alloc(8 * (size_t)P, st));
            HY_HIP(pk1.alloc(8 * (size_t)P, st));
            HY_HIP(pv0.alloc(4 * (size_t)P, st));
            HY_HIP(pv1.alloc(4 * (size_t)P, st));
            HY_HIP(mark.alloc(4 * (size_t)(P + 1), st));
            HY_HIP(run_start.alloc(4 * (size_t)P, st));
            HY_HIP(eoff.alloc(8 * (size_t)(P + 1), st));
            uint64_t *kk = pk0.as<uint64_t>(), *kka = pk1.as<uint64_t>();
            uint32_t *vv = pv0.as<uint32_t>(), *vva = pv1.as<uint32_t>();
            {
                hymet::ProfScope _ps(ctx, "sparse_postings", 20.0 * (double)P);
                HY_HIP(hipMemcpyAsync(d_poff.p, poff.data(), 8 * (size_t)(n_ids + 1), hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(sp_postings_kernel, dim3((unsigned)n_ids), dim3(kThreads), 0, st, d_ref_hashes, d_ref_off,
                                   n_side_ref, d_qry_hashes, d_qry_off, q_begin, d_poff.as<int64_t>(), (int)s, kk, vv);
                HY_CHECK_LAUNCH("sp_postings_kernel");
            }
            {
                hymet::ProfScope _ps(ctx, "sparse_sort_postings", 8.0 * 24.0 * (double)P);
                rc = hymet::mm::radix_sort_pairs(ctx, kk, kka, vv, vva, P, 0, 64);
                if (rc) return rc;
            }
            ids = vv;
            {
                hymet::ProfScope _ps(ctx, "sparse_count", 32.0 * (double)P);
                hipLaunchKernelGGL(sp_mark_kernel, dim3((unsigned)cdiv(P, kThreads)), dim3(kThreads), 0, st, kk, P,
                                   mark.as<int32_t>());
                HY_CHECK_LAUNCH("sp_mark_kernel");
                rc = hymet::mm::inclusive_max_scan_i32(ctx, mark.as<int32_t>(), run_start.as<int32_t>(), P, mpart);
                if (rc) return rc;
                // the marks are read; their buffer takes the counts
                const dim3 g((unsigned)cdiv(P + 1, kThreads));
                if (tri)
                    hipLaunchKernelGGL(sp_count_kernel<true>, g, dim3(kThreads), 0, st, ids, run_start.as<int32_t>(), P,
                                       first_q, mark.as<uint32_t>());
                else
                    hipLaunchKernelGGL(sp_count_kernel<false>, g, dim3(kThreads), 0, st, ids, run_start.as<int32_t>(), P,
                                       first_q, mark.as<uint32_t>());
                HY_CHECK_LAUNCH("sp_count_kernel");
                rc = hymet::mm::exclusive_scan_u32_i64(ctx, mark.as<uint32_t>(), eoff.as<int64_t>(), P + 1, &emitted);
                if (rc) return rc;
            }
        }
        counters->emitted = emitted;
        if (emitted > max_pairs || n_empty > max_pairs - emitted) {
            *total = -1;
            return hymet::fail(HYMET_E_CAPACITY, "hymet_mash_dist_sparse: " + std::to_string(emitted) + " pair keys and " +
                                                     std::to_string(n_empty) + " empty pairs, budget " +
                                                     std::to_string(max_pairs));
        }
        const int64_t N = emitted + n_empty;
        if (N == 0) return no_entries();
        HY_HIP(key0.alloc(8 * (size_t)N, st));
        HY_HIP(key1.alloc(8 * (size_t)N, st));
        hymet::ProfScope _ps(ctx, "sparse_emit", 12.0 * (double)N);
        if (emitted > 0) {
            hipLaunchKernelGGL(sp_emit_kernel, dim3((unsigned)cdiv(P, kThreads)), dim3(kThreads), 0, st, ids,
                               run_start.as<int32_t>(), eoff.as<int64_t>(), P, first_q, rb, key0.as<uint64_t>());
            HY_CHECK_LAUNCH("sp_emit_kernel");
        }
        if (n_empty > 0) {
            DevBuf d_eq, d_epre, d_er;
            HY_HIP(d_eq.alloc(4 * eq_row.size(), st));
            HY_HIP(d_epre.alloc(8 * epre.size(), st));
            HY_HIP(d_er.alloc(4 * er.size(), st));
            HY_HIP(hipMemcpyAsync(d_eq.p, eq_row.data(), 4 * eq_row.size(), hipMemcpyHostToDevice, st));
            HY_HIP(hipMemcpyAsync(d_epre.p, epre.data(), 8 * epre.size(), hipMemcpyHostToDevice, st));
            HY_HIP(hipMemcpyAsync(d_er.p, er.data(), 4 * er.size(), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(sp_empty_keys_kernel, dim3((unsigned)cdiv(n_empty, kThreads)), dim3(kThreads), 0, st,
                               d_eq.as<uint32_t>(), d_epre.as<int64_t>(), (int64_t)eq_row.size(), d_er.as<uint32_t>(), n_empty,
                               rb, key0.as<uint64_t>() + emitted);
            HY_CHECK_LAUNCH("sp_empty_keys_kernel");
        }
    }
    const int64_t N = emitted + n_empty;
    uint64_t *keys = key0.as<uint64_t>(), *keys_alt = key1.as<uint64_t>();
    {
        // the library's sort moves a value with every key: a byte nobody reads
        DevBuf b0, b1;
        HY_HIP(b0.alloc((size_t)N, st));
        HY_HIP(b1.alloc((size_t)N, st));
        uint8_t *bb = b0.as<uint8_t>(), *bba = b1.as<uint8_t>();
        hymet::ProfScope _ps(ctx, "sparse_sort_keys", (double)((kb + 7) / 8) * 18.0 * (double)N);
        rc = hymet::mm::radix_sort_pairs(ctx, keys, keys_alt, bb, bba, N, 0, kb);
        if (rc) return rc;
    }
    int64_t n_cand = 0;
    DevBuf cand;
    {
        DevBuf keep, kpos;
        HY_HIP(keep.alloc(4 * (size_t)(N + 1), st));
        HY_HIP(kpos.alloc(8 * (size_t)(N + 1), st));
        hymet::ProfScope _ps(ctx, "sparse_runs", 28.0 * (double)N);
        hipLaunchKernelGGL(sp_runs_kernel, dim3((unsigned)cdiv(N + 1, kThreads)), dim3(kThreads), 0, st, keys, N, (int)cmin, rb,
                           d_ref_off, d_qry_off, q_begin, n_empty > 0 ? 1 : 0, keep.as<uint32_t>());
        HY_CHECK_LAUNCH("sp_runs_kernel");
        rc = hymet::mm::exclusive_scan_u32_i64(ctx, keep.as<uint32_t>(), kpos.as<int64_t>(), N + 1, &n_cand);
        if (rc) return rc;
        counters->candidates = n_cand;
        if (n_cand == 0) return no_entries();
        HY_HIP(cand.alloc(8 * (size_t)n_cand, st));
        hipLaunchKernelGGL(sp_compact_kernel, dim3((unsigned)cdiv(N, kThreads)), dim3(kThreads), 0, st, keys,
                           keep.as<uint32_t>(), kpos.as<int64_t>(), N, cand.as<uint64_t>());
        HY_CHECK_LAUNCH("sp_compact_kernel");
    }
    key0.release();
    key1.release();
    HY_ARG(cdiv(n_cand, kWaves) < (1ll << 31), "hymet_mash_dist_sparse: more than 2^33 candidates in one call");
    DevBuf val, pass, ppos;
    HY_HIP(val.alloc(4 * (size_t)n_cand, st));
    HY_HIP(pass.alloc(4 * (size_t)(n_cand + 1), st));
    HY_HIP(ppos.alloc(8 * (size_t)(n_cand + 1), st));
    {
        hymet::ProfScope _ps(ctx, "sparse_exact", 16.0 * (double)s * (double)n_cand);
        HY_HIP(hipMemsetAsync(pass.as<uint32_t>() + n_cand, 0, 4, st));
        hipLaunchKernelGGL(sp_exact_kernel, dim3((unsigned)cdiv(n_cand, kWaves)), dim3(kThreads), 0, st, d_ref_hashes, d_ref_off,
                           d_qry_hashes, d_qry_off, q_begin, cand.as<uint64_t>(), n_cand, rb, (int)s, d_min_common,
                           val.as<uint32_t>(), pass.as<uint32_t>());
        HY_CHECK_LAUNCH("sp_exact_kernel");
    }
    hymet::ProfScope _ps(ctx, "sparse_csr", 24.0 * (double)n_cand + 8.0 * (double)rows);
    int64_t t = 0;
    rc = hymet::mm::exclusive_scan_u32_i64(ctx, pass.as<uint32_t>(), ppos.as<int64_t>(), n_cand + 1, &t);
    if (rc) return rc;
    *total = t;
    hipLaunchKernelGGL(sp_row_off_kernel, dim3((unsigned)cdiv(rows + 1, kThreads)), dim3(kThreads), 0, st, cand.as<uint64_t>(),
                       n_cand, rb, ppos.as<int64_t>(), rows, d_row_off);
    HY_CHECK_LAUNCH("sp_row_off_kernel");
    if (t > cap) {
        HY_HIP(hipStreamSynchronize(st));
        return hymet::fail(HYMET_E_CAPACITY, "hymet_mash_dist_sparse: " + std::to_string(t) + " entries, capacity " +
                                                 std::to_string(cap));
    }
    if (t > 0) {
        HY_ARG(d_ref_idx && d_val, "hymet_mash_dist_sparse: null output");
        hipLaunchKernelGGL(sp_write_kernel, dim3((unsigned)cdiv(n_cand, kThreads)), dim3(kThreads), 0, st, cand.as<uint64_t>(),
                           val.as<uint32_t>(), pass.as<uint32_t>(), ppos.as<int64_t>(), n_cand, rb, d_ref_idx, d_val);
        HY_CHECK_LAUNCH("sp_write_kernel");
    }
    HY_HIP(hipStreamSynchronize(st));
    return HYMET_OK;
}

int hymet_mash_dist_select(hymet_ctx *ctx, const uint32_t *d_block, int64_t n_rows, int64_t n_ref,
                           const uint16_t *d_min_common, int32_t s, int64_t *d_row_off, int32_t *d_ref_idx,
                           uint32_t *d_val, int64_t cap, int64_t *total) {
    HY_ARG(ctx && total, "hymet_mash_dist_select: null argument");
    *total = 0;
    HY_ARG(s >= 1 && s <= kMaxS, "hymet_mash_dist_select: sketch size must be in 1.." + std::to_string(kMaxS));
    HY_ARG(n_rows >= 0 && n_rows < (1ll << 31) - 1 && n_ref >= 0 && n_ref < (1ll << 31) && cap >= 0,
           "hymet_mash_dist_select: count out of range");
    HY_ARG(d_row_off && d_min_common, "hymet_mash_dist_select: null argument");
    HY_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (n_rows == 0 || n_ref == 0) {
        HY_HIP(hipMemsetAsync(d_row_off, 0, 8 * (size_t)(n_rows + 1), st));
        return HYMET_OK;
    }
    HY_ARG(d_block, "hymet_mash_dist_select: null block");
    hymet::mm::DevBuf cnt;
    HY_HIP(cnt.alloc(4 * (size_t)(n_rows + 1), st));
    hymet::ProfScope _ps(ctx, "mash_dist_select", 4.0 * (double)n_rows * (double)n_ref);
    HY_HIP(hipMemsetAsync(cnt.as<uint32_t>() + n_rows, 0, 4, st));  // the scan's last output is the total
    hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)n_rows), dim3(kThreads), 0, st, d_block, n_ref, d_min_common,
                       (int)s, cnt.as<uint32_t>());
    HY_CHECK_LAUNCH("select_count_kernel");
    int64_t t = 0;
    const int rc = hymet::mm::exclusive_scan_u32_i64(ctx, cnt.as<uint32_t>(), d_row_off, n_rows + 1, &t);  // synchronises
    if (rc) return rc;
    *total = t;
    if (t > cap)
        return hymet::fail(HYMET_E_CAPACITY, "hymet_mash_dist_select: " + std::to_string(t) + " entries, capacity " +
                                                 std::to_string(cap));
    if (t == 0) return HYMET_OK;
    HY_ARG(d_ref_idx && d_val, "hymet_mash_dist_select: null output");
    hipLaunchKernelGGL(select_write_kernel, dim3((unsigned)n_rows), dim3(kThreads), 0, st, d_block, n_ref, d_min_common,
                       (int)s, d_row_off, cap, d_ref_idx, d_val);
    HY_CHECK_LAUNCH("select_write_kernel");
    return HYMET_OK;
}

}  // extern "C"

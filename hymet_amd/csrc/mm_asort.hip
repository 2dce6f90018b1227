// Grouped anchor sort: the anchor words of a mapping batch (W = (rev | rid | rpos) << ybits | y,
// one 64-bit word per anchor; write_anchor_keys_kernel) into word order
// inside every query -- minimap2's radix sort of a query's anchors by x (map.c
// collect_seed_hits -> radix_sort_128x), with the canonical full (x, y) tie order T1
//  -- written out directly as the anchor set (x, y), so no unpack pass follows.
// The word holds everything the sort orders by and everything the anchor set needs: the
// query comes from the offsets, the span in y's high word is the batch's constant.  (Until
// the word, the emitter wrote a key q | rev | rid | rpos and a 32-bit y beside it: 12 B
// emitted, scattered and re-read per anchor, and packed into such a word by every block sort.)
//
// The words arrive query-major (one query's anchors are contiguous), so the global LSD sort
// over ~47 key bits (six 8-bit passes over 12 B per anchor) is replaced by work local to a
// query:
//   * a query of <= 4096 anchors is sorted whole in one block;
//   * a larger query is cut into tiles of 16384 anchors; every tile counts its anchors per
//     bin = (rev, rid) in LDS; a per-query scan turns the counts into each (tile, bin) run's
//     position and lists the non-empty bins -- the (query, strand, target) groups; the tiles
//     scatter their anchors to their runs, a bin's anchors staying in input order; every group
//     of <= 16384 anchors is then sorted by (rpos, y) in one block, and the larger groups (a
//     query against its own genome) by one device radix sort over all of them together (key =
//     group rank | key bits below the bin).
// A block sort keeps the word's bits that differ inside its segment (those below the bin for a
// group; the bits above go back on write-out).  The words
// are emitted minimizer by minimizer in query order, each minimizer's hits in index order, so
// inside a group they already rise in rpos (+ strand) or fall (- strand) but for stray hits
// elsewhere in the target (about 1 % of the anchors): the block first looks for that shape --
// a sorted backbone and at most 128 outliers, found by flagging both ends of every descent for
// up to three passes -- sorts the outliers in one wave and writes every word to its final
// place (block_seg_sort_kernel; HYMET_ASORT_ADAPT=0 turns this off).  Any other segment (a
// whole query, a shuffled group) is sorted in registers (bitonic, ITEMS per thread) and its
// runs merged in LDS: merge path splits, then each thread's outputs by a bitonic half-cleaner
// over two windows of ITEMS words (independent LDS loads instead of a serial merge).  The
// result is the same either way: the words are distinct up to identical (rpos, y) pairs.
// Segments of <= 64 anchors take a wave bitonic sort on the words, those of <= 8 a register
// network in one thread; class lists are filled with one global atomic per class and block.
// Equal keys after the device radix sort (one target position hit by several query
// minimizers) are put in y order on write.
// Index parts of more than 2047 targets use coarse bins of 2^cs consecutive targets (the
// bin histogram always fits LDS), sorted inside by (low target bits, rpos, y).  Where the word would
// not fit 63 bits (anchor_word_ybits; the stage then returns 1) the mapper emits no words: it
// takes its two-key fallback (mm_map.hip sort_anchor_set).
#include "mm_common.hpp"
#include "sort.hpp"

namespace hymet {
namespace mm {
namespace {

constexpr int kTile = 4096;     // largest query (or group) sorted whole in one block
// anchors per tile of a large query: the (tile, bin) count matrix is mostly zeros (a tile's
// anchors crowd into a few bins), so fewer, larger tiles cut its traffic (4096 -> 16384:
// query_scan / tile_hist touch a quarter of the rows)
constexpr int kPart = 16384;
constexpr int kMaxBins = 4096;  // (rev, rid) bins held in LDS

struct Seg {
    int64_t s;  // first anchor
    int32_t n;  // anchors
    int32_t q;  // query
};

// segment classes: thread (<= 8), wave (<= 64), blocks of 256 / 512 / 1024 / 2048 / 4096 and,
// for (query, strand, target) groups, 8192 / 16384 (a 1024-thread block sorting 16384 words in
// 136 KB of LDS), large
enum { kThread = 0, kWave, kB256, kB512, kB1K, kB2K, kB4K, kB8K, kB16K, kLarge, kClasses };

// queries: up to kTile sorted whole, larger ones tiled
__device__ __forceinline__ int seg_class(int64_t n) {
    return n <= 8 ? kThread : n <= 64 ? kWave : n <= 256 ? kB256 : n <= 512 ? kB512 : n <= 1024 ? kB1K : n <= 2048 ? kB2K
         : n <= kTile ? kB4K : kLarge;
}
// groups of a tiled query: whole up to 16384 (the device radix sort only above)
__device__ __forceinline__ int seg_class_group(int64_t n) {
    return n <= kTile ? seg_class(n) : n <= 8192 ? kB8K : n <= 16384 ? kB16K : kLarge;
}

// the anchor set written for sorted position i: x, y (the sorted key itself is not written),
// and the set's chaining-group heads: bit i of hb is set where the key above rpos -- (query,
// strand, target) -- differs from position i-1's, so chain_set numbers the groups from this
// bitmap instead of re-reading x (hb zeroed by grouped_anchor_sort; a word may straddle two
// writers' segments, hence the atomic)
struct AnchorOut {
    uint64_t *ax;
    uint32_t *ay;  // y's low word: the high word (the span) is the set's constant, kept beside the set
    int rb, pb, ybits;
    uint32_t *hb;
    uint32_t *ax32;  // x's low word (rpos) alone: the chaining kernels' reads, 4 B per anchor instead of 8
    // the anchor of word w = (rev | rid | rpos) << ybits | y
    __device__ __forceinline__ void put(int64_t i, uint64_t w) const {
        const uint64_t k = w >> ybits, y = w & ((1ull << ybits) - 1);
        const uint64_t rev = k >> (rb + pb) & 1, rid = k >> pb & ((1ull << rb) - 1), rpos = k & ((1ull << pb) - 1);
        ax[i] = rev << 63 | rid << 32 | rpos;
        ay[i] = (uint32_t)y;
        ax32[i] = (uint32_t)rpos;
    }
    // w written at i, wp at i - 1 (first: i starts a writer's segment -- a query or a bin, a
    // head either way)
    __device__ __forceinline__ void head(int64_t i, uint64_t w, uint64_t wp, bool first) const {
        if (first || (w >> (ybits + pb)) != (wp >> (ybits + pb))) atomicOr(hb + (i >> 5), 1u << (i & 31));
    }
};

// one slot per lane with `pred` in list cnt's range: one atomic per wave (every lane calls)
__device__ __forceinline__ int wave_append(int32_t *cnt, bool pred) {
    const uint64_t m = __ballot(pred);
    if (m == 0) return -1;
    const int lane = threadIdx.x & 63, leader = __ffsll((unsigned long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(cnt, __popcll(m));
    base = __shfl(base, leader, 64);
    return pred ? base + __popcll(m & ((1ull << lane) - 1)) : -1;
}

// Append the block's segments to their class lists: LDS counts per class, then one global
// atomic per class and block (a global atomic per item serialises on the 8 counters).
// ITEMS segments per thread; cls < 0: none.
template <int ITEMS>
__device__ __forceinline__ void block_append(const Seg (&sg)[ITEMS], const int (&cls)[ITEMS], Seg *lists, int64_t cap,
                                             int32_t *cnt) {
    __shared__ int32_t lc[kClasses], gb[kClasses];
    if (threadIdx.x < kClasses) lc[threadIdx.x] = 0;
    __syncthreads();
    int slot[ITEMS];
#pragma unroll
    for (int j = 0; j < ITEMS; j++) {
        slot[j] = -1;
        for (int k = 0; k < kClasses; k++) {
            const int sl = wave_append(&lc[k], cls[j] == k);
            if (sl >= 0) slot[j] = sl;
        }
    }
    __syncthreads();
    if (threadIdx.x < kClasses) gb[threadIdx.x] = lc[threadIdx.x] ? atomicAdd(&cnt[threadIdx.x], lc[threadIdx.x]) : 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < ITEMS; j++) {
        // the counters persist across calls (cleared by each kernel's last block): a stale
        // count must never write past a list; the host checks the totals against cap
        const int64_t at = cls[j] >= 0 ? (int64_t)gb[cls[j]] + slot[j] : cap;
        if (at < cap) lists[cls[j] * cap + at] = sg[j];
    }
}

// queries by size class (large: tiles counted)
__global__ __launch_bounds__(256) void query_class_kernel(const int64_t *qoff, int n_q, Seg *lists, int64_t cap, int32_t *cnt,
                                                          uint32_t *nt, int64_t *mail) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = q < n_q;
    const int64_t s = ok ? qoff[q] : 0, n = ok ? qoff[q + 1] - s : 0;
    if (ok) nt[q] = n > kTile ? (uint32_t)((n + kPart - 1) / kPart) : 0;
    const Seg sg[1] = {Seg{s, (int32_t)n, q}};
    const int cls[1] = {n > 0 ? seg_class(n) : -1};
    block_append<1>(sg, cls, lists, cap, cnt);
    publish_counters(cnt, kClasses, mail);
}

// LDS atomicAdd(&h[bin], 1) for the active lanes, returning the old values: the lanes of up
// to two bins shared by many lanes (a query's anchors crowd into its genome's bins) take one
// atomic per bin, the rest one each
__device__ __forceinline__ uint32_t lds_rank(uint32_t *h, int bin, bool active) {
    const int lane = threadIdx.x & 63;
    uint64_t pending = __ballot(active);
    uint32_t r = 0;
    for (int it = 0; it < 2 && pending; it++) {
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const int lb = __shfl(bin, leader, 64);
        const uint64_t m = __ballot(active && bin == lb) & pending;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&h[lb], (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, leader, 64);
        if (m >> lane & 1) r = base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        pending &= ~m;
    }
    if (pending >> lane & 1) r = atomicAdd(&h[bin], 1u);
    return r;
}

__global__ void tile_map_kernel(const Seg *large, int n_large, const int64_t *tpos, int64_t *tile_a0, int32_t *tile_q,
                                int32_t *tile_n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_large) return;
    const Seg S = large[i];
    int64_t t = tpos[S.q];
    for (int64_t a = 0; a < S.n; a += kPart, t++) {
        tile_a0[t] = S.s + a;
        tile_q[t] = S.q;
        tile_n[t] = (int32_t)min((int64_t)kPart, (int64_t)S.n - a);
    }
}

__global__ __launch_bounds__(256) void tile_hist_kernel(const uint64_t *__restrict__ key, const int64_t *__restrict__ tile_a0,
                                                        const int32_t *__restrict__ tile_n, int bsh, int nbins,
                                                        uint32_t *__restrict__ H) {
    __shared__ uint32_t h[kMaxBins];
    const int64_t a0 = tile_a0[blockIdx.x];
    const int n = tile_n[blockIdx.x];
    for (int b = threadIdx.x; b < nbins; b += 256) h[b] = 0;
    __syncthreads();
    // every lane runs the loop (wave-level ballots inside); eight rows of keys loaded at a time,
    // at clamped positions (straight-line loads: the waits are counted, not vmcnt(0) per row)
    for (int e0 = 0; e0 < n; e0 += 256 * 8) {
        uint64_t kv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) kv[u] = key[a0 + min(e0 + 256 * u + (int)threadIdx.x, n - 1)];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const bool act = e0 + 256 * u + (int)threadIdx.x < n;
            (void)lds_rank(h, act ? (int)((kv[u] >> bsh) & (nbins - 1)) : 0, act);
        }
    }
    __syncthreads();
    uint32_t *row = H + (int64_t)blockIdx.x * nbins;
    for (int b = threadIdx.x; b < nbins; b += 256) row[b] = h[b];
}

// one block per large query: H[t][b] <- offset (within the query) of tile t's bin-b run;
// every non-empty bin appended to the group list.  A thread per bin (rows of 1024 bins) walks
// the bin down the query's tiles: a long contig has hundreds of tiles, and its block is the
// launch's tail (256 threads walking four rows of bins one after the other took 1.3 ms per
// launch on C4)
__global__ __launch_bounds__(1024) void query_scan_kernel(const Seg *large, const int64_t *tpos, int nbins,
                                                          uint32_t *__restrict__ H, Seg *groups, int64_t cap,
                                                          int32_t *n_groups, int64_t *mail) {
    __shared__ uint32_t wsum[16], wgrp[16];
    __shared__ int32_t gbase;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const Seg S = large[blockIdx.x];
    const int64_t t0 = tpos[S.q], t1 = t0 + (S.n + kPart - 1) / kPart;
    uint32_t carry = 0;  // anchors in the bins of earlier rows (block-uniform)
    for (int r = 0; r < nbins; r += 1024) {  // bins r + tid, in bin order across rows
        const int b = r + tid;
        uint32_t run = 0;
        if (b < nbins)
            for (int64_t t = t0; t < t1; t += 32) {  // 32 loads in flight (clamped rows: straight-line)
                uint32_t v[32];
#pragma unroll
                for (int j = 0; j < 32; j++) v[j] = H[min(t + j, t1 - 1) * nbins + b];
#pragma unroll
                for (int j = 0; j < 32; j++)
                    if (t + j < t1) {
                        H[(t + j) * nbins + b] = run;  // exclusive within the bin, across tiles
                        run += v[j];
                    }
            }
        uint32_t inc = run;  // inclusive scan over the row's bins: waves, then the wave sums
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        uint32_t wex = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint32_t x = wsum[k];
            wex += k < w ? x : 0u;
            tot += x;
        }
        const uint32_t base = carry + wex + inc - run;
        carry += tot;
        if (b < nbins && run > 0)
            for (int64_t t = t0; t < t1; t += 32) {
                uint32_t v[32];
#pragma unroll
                for (int j = 0; j < 32; j++) v[j] = H[min(t + j, t1 - 1) * nbins + b];
#pragma unroll
                for (int j = 0; j < 32; j++)
                    if (t + j < t1) H[(t + j) * nbins + b] = v[j] + base;
            }
        // the row's non-empty bins appended with one global atomic per block (one per wave
        // serialised ~40k returning atomics per launch on the single counter)
        const bool ne = b < nbins && run > 0;
        const uint64_t nm = __ballot(ne);
        if (lane == 0) wgrp[w] = (uint32_t)__popcll(nm);
        __syncthreads();
        uint32_t gex = 0, gtot = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint32_t x = wgrp[k];
            gex += k < w ? x : 0u;
            gtot += x;
        }
        if (tid == 0) gbase = gtot ? atomicAdd(n_groups, (int32_t)gtot) : 0;
        __syncthreads();
        if (ne) {
            const int64_t slot = (int64_t)gbase + gex + __popcll(nm & ((1ull << lane) - 1));
            if (slot < cap) groups[slot] = Seg{S.s + base, (int32_t)run, S.q};  // host checks the total
        }
        __syncthreads();  // wsum / wgrp / gbase are rewritten by the next row
    }
    publish_counters(n_groups, 1, mail);
}

// The scatter of a large query's tile to its (tile, bin) runs.  Consecutive anchors of a tile
// fall into many bins (one minimizer hits every strain of the taxon), so writing each anchor
// straight to its run position scattered 12-byte writes over as many cache lines; instead each
// round of kSub anchors is ranked by bin in LDS (wave-aggregated atomics), its bin counts are
// scanned, the round is laid out bin by bin in LDS, and written run by run (consecutive lanes,
// consecutive addresses).
//
// A bin's anchors leave a round in input order (ORDERED): write_anchor_keys_kernel emits a
// group's anchors rising (+ strand) or falling (- strand) in rpos but for stray hits, and the
// block sorts' outlier path lives on that order.  Every wave ranks a contiguous quarter of the
// round into counters of its own -- its rows one after the other, a row's lanes of one bin in
// lane order (wave_rank_ordered) -- and a wave's ranks start after the earlier waves' counts.
// The counters are 16-bit (a round holds kSub < 65536 anchors) and wave-private, so they take
// plain loads and stores.  Unordered (the ranks of lds_rank, in the order the LDS serialises
// the waves' atomics) only where the ordered counters would pass 64 KB of LDS: 4096 bins.
// LDS per block: 8 B per round anchor + 4 B per bin + the rank counters, 8 B per bin ordered
// (four waves x 16 bits), 4 B unordered; sized to the part's bins at launch: 1024 bins and 2048
// anchors = 28 KB.  Four blocks per CU all the same: the ordered kernel's 122 VGPRs leave four
// waves per SIMD (the compiler's resource report; 36 KB, the size with key and value apart,
// gave the same four by LDS).  Measured on C4 with 12 B per anchor: 3072 anchors in a static
// 68 KB was 323 ms/step of mm_anchor_gsort, 44 KB dynamic 300, 2048 anchors in 32 KB 288
#ifndef HYMET_SCATTER_SUB
#define HYMET_SCATTER_SUB 2048
#endif
constexpr int kSub = HYMET_SCATTER_SUB;
static_assert(kSub % 256 == 0 && kSub < 65536, "scatter round: whole rows of 256, 16-bit ranks");

constexpr size_t scatter_lds(int nbins, bool ordered) { return (size_t)kSub * 8 + (size_t)nbins * (ordered ? 12 : 8); }
constexpr int kScatterWsum = 4;  // tile_scatter_kernel's static LDS: one scan word per wave
constexpr size_t kScatterStaticLds = kScatterWsum * sizeof(uint32_t);
// ordered ranking where its LDS, dynamic and static, fits the 64 KB a launch gets without
// opting in for more (4096 bins would take 65536 + 16 bytes: they stay unordered)
constexpr bool scatter_ordered(int nbins) { return scatter_lds(nbins, true) + kScatterStaticLds <= 65536; }
static_assert(scatter_ordered(2048) && !scatter_ordered(kMaxBins), "ordered scatter: up to 2048 bins");
static_assert(scatter_lds(kMaxBins, false) + kScatterStaticLds <= 65536, "unordered scatter LDS at the most bins");

// The rank of every active lane among the earlier anchors of its bin in the wave's part of the
// round, h[bin] counted up: the lanes of a row that share a bin find each other with one ballot
// per bin bit, rank in lane order, and their lowest lane updates the wave's counter.
__device__ __forceinline__ uint32_t wave_rank_ordered(uint16_t *h, int bin, bool active, int bin_bits) {
    const int lane = threadIdx.x & 63;
    uint64_t peers = __ballot(active);
    for (int i = 0; i < bin_bits; i++) {
        const bool bit = bin >> i & 1;
        const uint64_t m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    const int leader = active ? __ffsll((unsigned long long)peers) - 1 : lane;
    uint32_t base = 0;
    if (active && lane == leader) {
        base = h[bin];
        h[bin] = (uint16_t)(base + (uint32_t)__popcll(peers));
    }
    base = (uint32_t)__shfl((int)base, leader, 64);
    return base + (uint32_t)__popcll(peers & ((1ull << lane) - 1));
}

template <bool ORDERED>
__global__ __launch_bounds__(256) void tile_scatter_kernel(const uint64_t *__restrict__ key, const int64_t *__restrict__ tile_a0,
                                                           const int32_t *__restrict__ tile_q, const int32_t *__restrict__ tile_n,
                                                           const int64_t *__restrict__ qoff, int bsh, int nbins,
                                                           const uint32_t *__restrict__ H, uint64_t *__restrict__ okey) {
    extern __shared__ uint64_t smem[];
    uint64_t *sk = smem;                                   // [kSub]
    uint32_t *c = reinterpret_cast<uint32_t *>(sk + kSub);  // [nbins] run position of every bin for the next round
    // the round's bin counts, then their exclusive offsets; ordered: per wave, cw[w * nbins + b]
    uint32_t *lo = c + nbins;                              // [nbins] (unordered)
    uint16_t *cw = reinterpret_cast<uint16_t *>(lo);       // [4][nbins] (ordered)
    __shared__ uint32_t wsum[kScatterWsum];  // the kernel's only static LDS (kScatterStaticLds)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t a0 = tile_a0[blockIdx.x];
    const int n = tile_n[blockIdx.x];
    const uint32_t *row = H + (int64_t)blockIdx.x * nbins;
    for (int b = tid; b < nbins; b += 256) c[b] = row[b];
    const int64_t base = qoff[tile_q[blockIdx.x]];
    const int per = (nbins + 255) / 256, b0 = min(tid * per, nbins), b1 = min(b0 + per, nbins);
    const int bin_bits = 31 - __clz(nbins);
    // a thread's anchors of a round: ordered, row j of its wave's quarter; else row j of the round
    constexpr int kRows = kSub / 256;
    const int e_first = ORDERED ? w * (kSub / 4) + lane : tid, e_step = ORDERED ? 64 : 256;
    for (int r0 = 0; r0 < n; r0 += kSub) {
        const int m = min(kSub, n - r0);
        if (ORDERED) {
            for (int b = tid; b < 2 * nbins; b += 256) lo[b] = 0;  // cw, as words
        } else {
            for (int b = tid; b < nbins; b += 256) lo[b] = 0;
        }
        __syncthreads();
        uint64_t kk[kRows];
        uint32_t rk[kRows];
        int bn[kRows];
#pragma unroll
        for (int j = 0; j < kRows; j++) {  // the round's loads first, at clamped positions
            const int e = min(e_first + j * e_step, m - 1);
            kk[j] = key[a0 + r0 + e];
        }
#pragma unroll
        for (int j = 0; j < kRows; j++) {  // every lane runs the loop (wave-level ballots inside)
            const bool act = e_first + j * e_step < m;
            bn[j] = (int)((kk[j] >> bsh) & (uint64_t)(nbins - 1));
            rk[j] = ORDERED ? wave_rank_ordered(cw + w * nbins, act ? bn[j] : 0, act, bin_bits) : lds_rank(lo, bn[j], act);
        }
        __syncthreads();
        {  // exclusive scan of the bin counts: per-thread spans, then a block scan of span sums
            uint32_t sum = 0;
            for (int b = b0; b < b1; b++) {
                if (ORDERED) sum += (uint32_t)cw[b] + cw[nbins + b] + cw[2 * nbins + b] + cw[3 * nbins + b];
                else sum += lo[b];
            }
            uint32_t inc = sum;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
                if (lane >= d) inc += o;
            }
            if (lane == 63) wsum[w] = inc;
            __syncthreads();
            uint32_t ex = inc - sum;
            for (int k = 0; k < w; k++) ex += wsum[k];
            for (int b = b0; b < b1; b++) {
                if (ORDERED) {  // wave k's anchors of the bin after those of the waves before it
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const uint32_t t = cw[k * nbins + b];
                        cw[k * nbins + b] = (uint16_t)ex;
                        ex += t;
                    }
                } else {
                    const uint32_t t = lo[b];
                    lo[b] = ex;
                    ex += t;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kRows; j++)
            if (e_first + j * e_step < m) {
                const uint32_t slot = (ORDERED ? (uint32_t)cw[w * nbins + bn[j]] : lo[bn[j]]) + rk[j];
                sk[slot] = kk[j];
            }
        __syncthreads();
        // the bin's first slot of the round: the first wave's offset where ordered
        for (int s = tid; s < m; s += 256) {
            const uint64_t k = sk[s];
            const int b = (int)((k >> bsh) & (uint64_t)(nbins - 1));
            const int64_t pos = base + c[b] + (s - (ORDERED ? (uint32_t)cw[b] : lo[b]));
            okey[pos] = k;
        }
        __syncthreads();
        for (int b = tid; b < nbins; b += 256) {
            const uint32_t cur = ORDERED ? (uint32_t)cw[b] : lo[b];
            const uint32_t nxt = b + 1 < nbins ? (ORDERED ? (uint32_t)cw[b + 1] : lo[b + 1]) : (uint32_t)m;
            c[b] += nxt - cur;
        }
        __syncthreads();
    }
}

// groups by size class, 4 per thread; a single-anchor group is final where the scatter put it
__global__ __launch_bounds__(256) void group_class_kernel(const Seg *groups, int64_t G, Seg *lists, int64_t cap, int32_t *cnt,
                                                          const uint64_t *key, AnchorOut out, int64_t *mail) {
    Seg sg[4];
    int cls[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t g = (int64_t)blockIdx.x * 1024 + j * 256 + threadIdx.x;
        sg[j] = g < G ? groups[g] : Seg{0, 0, 0};
        if (sg[j].n == 1) {
            const uint64_t k = key[sg[j].s];
            out.put(sg[j].s, k);
            out.head(sg[j].s, k, k, true);
        }
        cls[j] = sg[j].n > 1 ? seg_class_group(sg[j].n) : -1;
    }
    block_append<4>(sg, cls, lists, cap, cnt);
    publish_counters(cnt, kClasses, mail);
}

// one thread per segment of <= 8 anchors: sorting network on the words in registers
__global__ __launch_bounds__(256) void thread_seg_sort_kernel(const Seg *list, int n_seg, const uint64_t *key, AnchorOut out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_seg) return;
    const Seg S = list[i];
    uint64_t k[8];
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = j < S.n ? key[S.s + j] : ~0ull;
#pragma unroll
    for (int w = 2; w <= 8; w <<= 1)
#pragma unroll
        for (int d = w >> 1; d > 0; d >>= 1)
#pragma unroll
            for (int a = 0; a < 8; a++) {
                const int b = a ^ d;
                if (b > a) {
                    const bool up = (a & w) == 0;
                    if ((k[a] > k[b]) == up) {
                        const uint64_t tk = k[a];
                        k[a] = k[b];
                        k[b] = tk;
                    }
                }
            }
#pragma unroll
    for (int j = 0; j < 8; j++)
        if (j < S.n) {
            out.put(S.s + j, k[j]);
            out.head(S.s + j, k[j], k[j > 0 ? j - 1 : 0], j == 0);
        }
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
    const int lo = __shfl_xor((int)(uint32_t)v, m, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return (uint64_t)(uint32_t)hi << 32 | (uint32_t)lo;
}

// one wave per segment of <= 64 anchors: bitonic sort on the words in registers
__global__ __launch_bounds__(64) void wave_seg_sort_kernel(const Seg *list, const uint64_t *key, AnchorOut out) {
    const Seg S = list[blockIdx.x];
    const int lane = threadIdx.x;
    uint64_t k = lane < S.n ? key[S.s + lane] : ~0ull;
    for (int w = 2; w <= 64; w <<= 1)
        for (int j = w >> 1; j > 0; j >>= 1) {
            const uint64_t ok = shfl_xor64(k, j);
            const bool up = (lane & w) == 0, lower = (lane & j) == 0;
            if ((lower == up) == (ok < k)) k = ok;  // the lower lane of an ascending pair keeps the min
        }
    const uint64_t kp = (uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(k >> 32), 1, 64) << 32 |
                        (uint32_t)__shfl_up((int)(uint32_t)k, 1, 64);  // lane - 1's word
    if (lane < S.n) {
        out.put(S.s + lane, k);
        out.head(S.s + lane, k, kp, lane == 0);
    }
}

__device__ __forceinline__ int lds_ix(int e) { return e + (e >> 4); }  // one pad word per 16: blocked access without bank conflicts

// ascending bitonic network over a thread's N words (unrolled: registers only)
template <int N>
__device__ __forceinline__ void reg_sort(uint64_t (&k)[N]) {
#pragma unroll
    for (int w = 2; w <= N; w <<= 1)
#pragma unroll
        for (int j = w >> 1; j > 0; j >>= 1)
#pragma unroll
            for (int i = 0; i < N; i++) {
                const int l = i ^ j;
                if (l > i) {
                    const uint64_t a = k[i], b = k[l];
                    const bool up = (i & w) == 0;
                    k[i] = up ? min(a, b) : max(a, b);
                    k[l] = up ? max(a, b) : min(a, b);
                }
            }
}

// most outliers the outlier path of a block sort takes: one wave sorts them, one or two words
// per lane (A/B knob, 64 or 128; measured: 64 finishes 96.3 % of the block-sorted anchors of
// C4 and 69.9 % of the Zymo-backbone workload's, 128 98.5 % and 84.7 %)
#ifndef HYMET_ASORT_OUTMAX
#define HYMET_ASORT_OUTMAX 128
#endif
constexpr int kOutMax = HYMET_ASORT_OUTMAX;
static_assert(kOutMax == 64 || kOutMax == 128, "the outlier sort holds one or two words per lane");
// what the block sorts did, counted where the caller asks (hymet_mm_anchor_sort): segments and
// anchors finished by the outlier path, segments and anchors that took the full sort
enum { kStFastSegs = 0, kStFastAnchors, kStFullSegs, kStFullAnchors, kStats };

// first position in the ascending o[lo, hi) whose word is not below x
__device__ __forceinline__ int lower_bound64(const uint64_t *o, int lo, int hi, uint64_t x) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (o[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one block of BLOCK threads per segment of <= BLOCK * ITEMS anchors: the words' low wbits
// bits (the rest is the segment's constant) sorted by register networks + LDS merge path.
//
// Before that, the outlier path (adapt): a (query, strand, target) group arrives as a rising
// -- on the - strand falling -- backbone plus a few stray hits, so the segment, read back to
// front where its first word is above its last, is split into a sorted rest and <= kOutMax
// outliers: both ends of every descent are flagged, then both ends of every descent among the
// words still unflagged, for at most three such passes; a pass that flags nothing proves the
// rest sorted.  One wave sorts the outliers, and every word goes straight to its final place:
// a kept word to its rank among the kept words plus the outliers below it, an outlier to its
// rank among the outliers plus the kept words not above it (kept before outlier on a tie).
// The cost does not depend on the class's padded capacity.  A segment that is not of that
// shape (a whole query, a shuffled group) takes the full sort from the words already staged.
template <int BLOCK, int ITEMS>
__global__ __launch_bounds__(BLOCK) void block_seg_sort_kernel(const Seg *list, const uint64_t *key, int wbits, AnchorOut out,
                                                               int adapt, unsigned long long *stats) {
    constexpr int CAP = BLOCK * ITEMS;
    static_assert(ITEMS <= 16 && BLOCK % 64 == 0, "flag words hold 16 bits per thread; whole waves");
    __shared__ uint64_t sm[CAP + CAP / 16];
    // outlier path: per thread, the flags of its words (low half) and those other threads set
    // in the running pass (high half); words flagged per pass; outliers; wave sums
    __shared__ uint32_t fmw[BLOCK], pcnt[4], wsum[BLOCK / 64];
    __shared__ uint64_t ol[kOutMax];
    const Seg S = list[blockIdx.x];
    const int tid = threadIdx.x;
    const uint64_t lm = (1ull << wbits) - 1;  // the word's bits that differ inside the segment
    const uint64_t hi_bits = key[S.s] & ~lm;
    fmw[tid] = 0;
    if (tid < 4) pcnt[tid] = 0;
    {  // coalesced load, striped: every row's loads issued before any is used (clamped positions)
        uint64_t kr[ITEMS];
#pragma unroll
        for (int u = 0; u < ITEMS; u++) kr[u] = key[S.s + min(u * BLOCK + tid, S.n - 1)];
#pragma unroll
        for (int u = 0; u < ITEMS; u++) {
            const int e = u * BLOCK + tid;
            sm[lds_ix(e)] = e < S.n ? (kr[u] & lm) : ~0ull;
        }
    }
    __syncthreads();
    uint64_t k[ITEMS];
    bool done = false;  // block-uniform: the outlier path has every word at its place in sm
    if (adapt) {
        const int n = S.n;
        const bool rev = sm[0] > sm[lds_ix(n - 1)];
        // word e of the segment in the order the path reads it; past its end, the padding
        auto at = [&](int e) -> uint64_t { return e < n ? sm[lds_ix(rev ? n - 1 - e : e)] : ~0ull; };
#pragma unroll
        for (int j = 0; j < ITEMS; j++) k[j] = at(tid * ITEMS + j);
        constexpr uint32_t kFull = (1u << ITEMS) - 1;
        uint32_t fl = 0;        // the thread's flagged words
        int total = 0;          // the block's
        uint64_t prev = 0;      // the last unflagged word before the thread's own
        bool has_prev = false;
        // passes 0..2 flag, a pass that finds nothing to flag ends the search; pass 3 only checks
        for (int p = 0; p < 4; p++) {
            int pt = -1, pj = 0;
            for (int t = tid - 1; t >= 0; t--) {  // bounded: <= kOutMax words are flagged
                const uint32_t m = fmw[t] & kFull;
                if (m != kFull) {
                    pt = t;
                    pj = 31 - __clz((int)(~m & kFull));
                    break;
                }
            }
            has_prev = pt >= 0;
            prev = has_prev ? at(pt * ITEMS + pj) : 0;
            uint32_t nf = 0;
            uint64_t cur = prev;
            int ct = pt, cj = pj;
#pragma unroll
            for (int j = 0; j < ITEMS; j++)
                if (!(fl >> j & 1)) {
                    if (ct >= 0 && k[j] < cur) {  // a descent: both ends
                        nf |= 1u << j;
                        if (ct == tid) nf |= 1u << cj;
                        else atomicOr(&fmw[ct], 0x10000u << cj);
                    }
                    cur = k[j];
                    ct = tid;
                    cj = j;
                }
            __syncthreads();
            nf |= fmw[tid] >> 16;
            fl |= nf;
            fmw[tid] = fl;
            if (nf) atomicAdd(&pcnt[p], (uint32_t)__popc(nf));
            __syncthreads();
            const int cn = (int)pcnt[p];
            if (cn == 0) {
                done = true;
                break;
            }
            total += cn;
            if (total > kOutMax) break;
        }
        if (done && total > 0) {
            const int lane = tid & 63, w = tid >> 6;
            const uint32_t c = (uint32_t)__popc(fl);
            uint32_t inc = c;  // flagged words before the thread's own: waves, then the wave sums
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
                if (lane >= d) inc += o;
            }
            if (lane == 63) wsum[w] = inc;
            __syncthreads();
            uint32_t fb = inc - c;
            for (int i = 0; i < w; i++) fb += wsum[i];
#pragma unroll
            for (int j = 0; j < ITEMS; j++)
                if (fl >> j & 1) ol[fb + (uint32_t)__popc(fl & ((1u << j) - 1))] = k[j];
            __syncthreads();
            if (tid < 64 && total <= 64) {  // the first wave sorts the outliers (bitonic, a word per lane)
                uint64_t v = tid < total ? ol[tid] : ~0ull;
                for (int ww = 2; ww <= 64; ww <<= 1)
                    for (int j = ww >> 1; j > 0; j >>= 1) {
                        const uint64_t ov = shfl_xor64(v, j);
                        const bool up = (tid & ww) == 0, lower = (tid & j) == 0;
                        if ((lower == up) == (ov < v)) v = ov;
                    }
                ol[tid] = v;
            } else if (kOutMax > 64 && tid < 64) {  // two words per lane: elements tid and tid + 64
                uint64_t v[2] = {ol[tid], tid + 64 < total ? ol[(tid + 64) % kOutMax] : ~0ull};
                for (int ww = 2; ww <= 128; ww <<= 1)
                    for (int j = ww >> 1; j > 0; j >>= 1) {
                        if (j == 64) {  // the last merge's first step: within the lane, ascending
                            const uint64_t a = min(v[0], v[1]), b = max(v[0], v[1]);
                            v[0] = a;
                            v[1] = b;
                            continue;
                        }
#pragma unroll
                        for (int r = 0; r < 2; r++) {
                            const uint64_t ov = shfl_xor64(v[r], j);
                            const bool up = ((tid + 64 * r) & ww) == 0, lower = (tid & j) == 0;
                            if ((lower == up) == (ov < v[r])) v[r] = ov;
                        }
                    }
                ol[tid] = v[0];
                ol[(tid + 64) % kOutMax] = v[1];
            }
            __syncthreads();
            // Every word to its place.  lcur: outliers below the last kept word handled so far; a
            // kept word of rank r (among the kept) with lj outliers below it goes to r + lj, and
            // the outliers [lcur, lj) -- not below its predecessor, below it -- to their index + r.
            int lcur = has_prev ? lower_bound64(ol, 0, total, prev) : 0;
            const uint32_t kept = ~fl & kFull;
            if (kept) {
                uint64_t last = 0;
#pragma unroll
                for (int j = 0; j < ITEMS; j++)
                    if (kept >> j & 1) last = k[j];
                const int lend = lower_bound64(ol, lcur, total, last);
                int r = tid * ITEMS - (int)fb;
#pragma unroll
                for (int j = 0; j < ITEMS; j++)
                    if (kept >> j & 1) {
                        const int lj = lcur == lend ? lcur : lower_bound64(ol, lcur, lend, k[j]);
                        for (int i = lcur; i < lj; i++) sm[lds_ix(i + r)] = ol[i];
                        sm[lds_ix(r + lj)] = k[j];
                        lcur = lj;
                        r++;
                    }
            }
            // outliers above every kept word (a full segment: no padding above them)
            if (tid == BLOCK - 1)
                for (int i = lcur; i < total; i++) sm[lds_ix(i + CAP - total)] = ol[i];
        } else if (done && rev) {
#pragma unroll
            for (int j = 0; j < ITEMS; j++) sm[lds_ix(tid * ITEMS + j)] = k[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < ITEMS; j++) k[j] = sm[lds_ix(tid * ITEMS + j)];
    }
    if (stats && tid == 0) {
        atomicAdd(stats + (done ? kStFastSegs : kStFullSegs), 1ull);
        atomicAdd(stats + (done ? kStFastAnchors : kStFullAnchors), (unsigned long long)S.n);
    }
    if (!done) {  // the full sort: register networks, then merge rounds
        reg_sort<ITEMS>(k);
        for (int run = ITEMS; run < CAP; run <<= 1) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < ITEMS; j++) sm[lds_ix(tid * ITEMS + j)] = k[j];
            __syncthreads();
            const int o = tid * ITEMS, base = o & ~(2 * run - 1), diag = o - base;
            const int a0 = base, b0 = base + run;
            int lo = max(0, diag - run), hi = min(diag, run);
            while (lo < hi) {  // merge path: first lo with A[lo] > B[diag - 1 - lo]
                const int mid = (lo + hi) >> 1;
                if (sm[lds_ix(a0 + mid)] <= sm[lds_ix(b0 + diag - 1 - mid)]) lo = mid + 1;
                else hi = mid;
            }
            // the thread's ITEMS outputs are the ITEMS smallest of A[ai..] and B[bi..]: min(A[ai + j],
            // B[bi + ITEMS-1-j]) holds exactly those as a bitonic sequence -- independent LDS
            // loads and a half-cleaner network instead of a serial merge
            const int ai = a0 + lo, bi = b0 + diag - lo;
            const int ae = a0 + run, be = b0 + run;
#pragma unroll
            for (int j = 0; j < ITEMS; j++) {
                const int ia = ai + j, ib = bi + ITEMS - 1 - j;
                const uint64_t va = ia < ae ? sm[lds_ix(ia)] : ~0ull, vb = ib < be ? sm[lds_ix(ib)] : ~0ull;
                k[j] = min(va, vb);
            }
#pragma unroll
            for (int d = ITEMS >> 1; d > 0; d >>= 1)
#pragma unroll
                for (int i = 0; i < ITEMS; i++)
                    if ((i & d) == 0) {
                        const uint64_t x = k[i], y = k[i + d];
                        k[i] = min(x, y);
                        k[i + d] = max(x, y);
                    }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < ITEMS; j++) sm[lds_ix(tid * ITEMS + j)] = k[j];
    }
    __syncthreads();
    for (int e = tid; e < S.n; e += BLOCK) {  // coalesced write
        const uint64_t w = sm[lds_ix(e)], wp = sm[lds_ix(e > 0 ? e - 1 : 0)];
        out.put(S.s + e, hi_bits | w);
        out.head(S.s + e, hi_bits | w, hi_bits | wp, e == 0);
    }
}

// groups above 4096 anchors: gathered as (rank << pb | rpos, y), sorted together, put back
__global__ __launch_bounds__(256) void big_gather_kernel(const Seg *list, const int64_t *dst, int pb, int ybits,
                                                         const uint64_t *key, uint64_t *tk, uint32_t *tv) {
    const Seg S = list[blockIdx.x];
    const int64_t d = dst[blockIdx.x];
    const uint64_t pm = (1ull << pb) - 1, ym = (1ull << ybits) - 1;
    for (int e = threadIdx.x; e < S.n; e += 256) {
        const uint64_t w = key[S.s + e];
        tk[d + e] = (uint64_t)blockIdx.x << pb | (w >> ybits & pm);
        tv[d + e] = (uint32_t)(w & ym);
    }
}

// sorted big groups back into place; runs of equal key take their y values in order
// (insertion sort by the run's first lane; such runs are short and rare)
__global__ __launch_bounds__(256) void big_put_kernel(const Seg *list, const int64_t *dst, int pb, int ybits,
                                                      const uint64_t *key, const uint64_t *tk, const uint32_t *tv, AnchorOut out) {
    const Seg S = list[blockIdx.x];
    const int64_t d = dst[blockIdx.x];
    const uint64_t pm = (1ull << pb) - 1;
    const uint64_t hi_bits = key[S.s] & ~((1ull << (pb + ybits)) - 1);  // the group's word bits above the sorted ones
    auto word = [&](uint64_t k, uint32_t y) -> uint64_t { return hi_bits | (k & pm) << ybits | y; };
    for (int e = threadIdx.x; e < S.n; e += 256) {
        const uint64_t k = tk[d + e];
        const bool prev_eq = e > 0 && tk[d + e - 1] == k;
        if (prev_eq) continue;
        out.head(S.s + e, word(k, 0), word(tk[d + (e > 0 ? e - 1 : 0)], 0), e == 0);
        int f = e;
        while (f + 1 < S.n && tk[d + f + 1] == k) f++;
        if (f == e) {
            out.put(S.s + e, word(k, tv[d + e]));
            continue;
        }
        uint32_t ys[64];
        const int m = min(f - e + 1, 64);
        for (int a = 0; a < m; a++) {
            const uint32_t v = tv[d + e + a];
            int b = a;
            while (b > 0 && ys[b - 1] > v) {
                ys[b] = ys[b - 1];
                b--;
            }
            ys[b] = v;
        }
        for (int a = 0; a < m; a++) out.put(S.s + e + a, word(k, ys[a]));
        for (int a = m; a <= f - e; a++) out.put(S.s + e + a, word(k, tv[d + e + a]));  // > 64 equal keys: input order
    }
}

__global__ void seg_len_kernel(const Seg *list, int n, uint32_t *len) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) len[i] = (uint32_t)list[i].n;
}

int bits_of(int64_t v) {
    int b = 1;
    while ((1ll << b) <= v) b++;
    return b;
}

// the stage's test entry: a caller's (q | rev | rid | rpos, y) pairs as anchor words
__global__ void pack_words_kernel(const uint64_t *key, const uint32_t *val, int64_t n, int kbits, int ybits, uint64_t *w) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) w[i] = (key[i] & ((1ull << kbits) - 1)) << ybits | val[i];
}

// sort the segments of `lists` (class-major, capacity cap; counts hc), all but the large class
// (wbits: the word's bits below the segment's common ones)
int sort_segments(hymet_ctx *ctx, const Seg *lists, int64_t cap, const int32_t *hc, const uint64_t *key, int wbits,
                  const AnchorOut &out, unsigned long long *stats) {
    hipStream_t st = ctx->stream;
    // HYMET_ASORT_ADAPT=0: the block sorts without their outlier path (A/B timing, tests)
    const int adapt = env_flag("HYMET_ASORT_ADAPT", true) ? 1 : 0;
#define HY_SEG_LAUNCH(cls, kern, block)                                                                                     \
    if (hc[cls] > 0) {                                                                                                      \
        hipLaunchKernelGGL(kern, dim3((unsigned)hc[cls]), dim3(block), 0, st, lists + cls * cap, key, wbits, out, adapt,    \
                           stats);                                                                                          \
        HY_CHECK_LAUNCH(#kern);                                                                                             \
    }
    if (hc[kThread] > 0) {
        hipLaunchKernelGGL(thread_seg_sort_kernel, dim3((unsigned)cdiv(hc[kThread], 256)), dim3(256), 0, st, lists + kThread * cap,
                           hc[kThread], key, out);
        HY_CHECK_LAUNCH("thread_seg_sort_kernel");
    }
    if (hc[kWave] > 0) {
        hipLaunchKernelGGL(wave_seg_sort_kernel, dim3((unsigned)hc[kWave]), dim3(64), 0, st, lists + kWave * cap, key, out);
        HY_CHECK_LAUNCH("wave_seg_sort_kernel");
    }
    HY_SEG_LAUNCH(kB256, (block_seg_sort_kernel<64, 4>), 64)
    HY_SEG_LAUNCH(kB512, (block_seg_sort_kernel<64, 8>), 64)
    // (A/B knobs: threads per block of the 1K / 2K / 4K / 8K classes; items = class size / threads)
#ifndef HYMET_SORT_T1K
#define HYMET_SORT_T1K 64
#endif
#ifndef HYMET_SORT_T2K
#define HYMET_SORT_T2K 128
#endif
#ifndef HYMET_SORT_T4K
#define HYMET_SORT_T4K 256
#endif
#ifndef HYMET_SORT_T8K
#define HYMET_SORT_T8K 512
#endif
    HY_SEG_LAUNCH(kB1K, (block_seg_sort_kernel<HYMET_SORT_T1K, 1024 / HYMET_SORT_T1K>), HYMET_SORT_T1K)
    HY_SEG_LAUNCH(kB2K, (block_seg_sort_kernel<HYMET_SORT_T2K, 2048 / HYMET_SORT_T2K>), HYMET_SORT_T2K)
    HY_SEG_LAUNCH(kB4K, (block_seg_sort_kernel<HYMET_SORT_T4K, 4096 / HYMET_SORT_T4K>), HYMET_SORT_T4K)
    HY_SEG_LAUNCH(kB8K, (block_seg_sort_kernel<HYMET_SORT_T8K, 8192 / HYMET_SORT_T8K>), HYMET_SORT_T8K)
    HY_SEG_LAUNCH(kB16K, (block_seg_sort_kernel<1024, 16>), 1024)
#undef HY_SEG_LAUNCH
    return HYMET_OK;
}

}  // namespace

int grouped_anchor_sort(hymet_ctx *ctx, const uint64_t *key, int64_t n, const int64_t *d_qoff, int n_q, int rb, int pb,
                        int64_t max_qlen, uint64_t *okey, uint64_t *ax, uint32_t *ay, uint32_t *hb,
                        uint32_t *ax32, unsigned long long *d_stats) {
    // bins = (strand, target) -- or, for parts of more than 2047 targets, (strand, target >> cs):
    // coarse bins of 2^cs consecutive targets, sorted inside by (low target bits, rpos, y)
    const int cs = std::max(0, 1 + rb - 12);
    const int nbins = 1 << (1 + rb - cs);
    const int gb = pb + cs;  // key bits below the bin
    const int ybits = anchor_word_ybits(rb, pb, max_qlen);
    if (n <= 0 || n_q <= 0 || ybits == 0) return 1;
    hipStream_t st = ctx->stream;
    const AnchorOut out{ax, ay, rb, pb, ybits, hb, ax32};
    HY_HIP(hipMemsetAsync(hb, 0, head_bits_bytes(n), st));
    // 1 queries by size
    DevBuf qlists, nt;
    HY_HIP(qlists.alloc(sizeof(Seg) * kClasses * (size_t)n_q, st));
    HY_HIP(nt.alloc(4 * (size_t)(n_q + 1), st));
    hipLaunchKernelGGL(query_class_kernel, dim3((unsigned)cdiv(n_q, 256)), dim3(256), 0, st, d_qoff, n_q, qlists.as<Seg>(),
                       (int64_t)n_q, ctx->dctr + kCtrQClass, nt.as<uint32_t>(), mb_dev(ctx, kMbQClass));
    HY_CHECK_LAUNCH("query_class_kernel");
    HY_HIP(hipStreamSynchronize(st));
    int32_t hq[kClasses] = {};
    for (int c = 0; c < kClasses; c++) {
        hq[c] = (int32_t)mb_read(ctx, kMbQClass + c);
        if (hq[c] < 0 || hq[c] > n_q) return hymet::fail(HYMET_E_INTERNAL, "grouped_anchor_sort: query class count > cap");
    }
    // word read by the histogram and by the scatter, scatter write, sort read, x + y (4 B) + x32 write
    ProfScope _ps(ctx, "mm_anchor_gsort", 48.0 * (double)n);
    // 2 small queries: sorted whole
    int rc = sort_segments(ctx, qlists.as<Seg>(), n_q, hq, key, 1 + rb + pb + ybits, out, d_stats);
    if (rc || hq[kLarge] == 0) return rc;
    // 3 large queries: tiles, bin histograms, per-query scan, scatter
    const int nl = hq[kLarge];
    const Seg *large = qlists.as<Seg>() + kLarge * (size_t)n_q;
    DevBuf tpos;
    HY_HIP(tpos.alloc(8 * (size_t)(n_q + 1), st));
    int64_t NT = 0;
    rc = exclusive_scan_u32_i64(ctx, nt.as<uint32_t>(), tpos.as<int64_t>(), n_q, &NT);
    if (rc) return rc;
    DevBuf ta0, tq, tn, H;
    HY_HIP(ta0.alloc(8 * (size_t)NT, st));
    HY_HIP(tq.alloc(4 * (size_t)NT, st));
    HY_HIP(tn.alloc(4 * (size_t)NT, st));
    HY_HIP(H.alloc(4 * (size_t)NT * nbins, st));
    hipLaunchKernelGGL(tile_map_kernel, dim3((unsigned)cdiv(nl, 256)), dim3(256), 0, st, large, nl, tpos.as<int64_t>(),
                       ta0.as<int64_t>(), tq.as<int32_t>(), tn.as<int32_t>());
    HY_CHECK_LAUNCH("tile_map_kernel");
    hipLaunchKernelGGL(tile_hist_kernel, dim3((unsigned)NT), dim3(256), 0, st, key, ta0.as<int64_t>(), tn.as<int32_t>(),
                       gb + ybits, nbins, H.as<uint32_t>());
    HY_CHECK_LAUNCH("tile_hist_kernel");
    const int64_t gcap = std::min<int64_t>(n, NT * (int64_t)nbins);  // a group holds >= 1 anchor
    HY_ARG(gcap < INT32_MAX, "grouped_anchor_sort: too many groups in one batch");
    DevBuf groups;
    HY_HIP(groups.alloc(sizeof(Seg) * (size_t)(gcap + 1), st));
    hipLaunchKernelGGL(query_scan_kernel, dim3((unsigned)nl), dim3(1024), 0, st, large, tpos.as<int64_t>(), nbins,
                       H.as<uint32_t>(), groups.as<Seg>(), gcap, ctx->dctr + kCtrGroups, mb_dev(ctx, kMbGroups));
    HY_CHECK_LAUNCH("query_scan_kernel");
    HY_ARG(nbins >= 1 && nbins <= kMaxBins, "grouped_anchor_sort: bin count out of range");
    if (scatter_ordered(nbins))
        hipLaunchKernelGGL(tile_scatter_kernel<true>, dim3((unsigned)NT), dim3(256), scatter_lds(nbins, true), st, key,
                           ta0.as<int64_t>(), tq.as<int32_t>(), tn.as<int32_t>(), d_qoff, gb + ybits, nbins, H.as<uint32_t>(), okey);
    else
        hipLaunchKernelGGL(tile_scatter_kernel<false>, dim3((unsigned)NT), dim3(256), scatter_lds(nbins, false), st, key,
                           ta0.as<int64_t>(), tq.as<int32_t>(), tn.as<int32_t>(), d_qoff, gb + ybits, nbins, H.as<uint32_t>(), okey);
    HY_CHECK_LAUNCH("tile_scatter_kernel");
    // 4 groups of the large queries, sorted in place by (rpos, y)
    HY_HIP(hipStreamSynchronize(st));
    const int32_t G = (int32_t)mb_read(ctx, kMbGroups);
    if (G == 0) return HYMET_OK;
    if (G < 0 || G > gcap) return hymet::fail(HYMET_E_INTERNAL, "grouped_anchor_sort: group count > cap");
    DevBuf glists;
    HY_HIP(glists.alloc(sizeof(Seg) * kClasses * (size_t)G, st));
    hipLaunchKernelGGL(group_class_kernel, dim3((unsigned)cdiv(G, 1024)), dim3(256), 0, st, groups.as<Seg>(), (int64_t)G,
                       glists.as<Seg>(), (int64_t)G, ctx->dctr + kCtrGClass, okey, out, mb_dev(ctx, kMbGClass));
    HY_CHECK_LAUNCH("group_class_kernel");
    HY_HIP(hipStreamSynchronize(st));
    int32_t hg[kClasses] = {};
    for (int c = 0; c < kClasses; c++) {
        hg[c] = (int32_t)mb_read(ctx, kMbGClass + c);
        if (hg[c] < 0 || hg[c] > G) return hymet::fail(HYMET_E_INTERNAL, "grouped_anchor_sort: group class count > cap");
    }
    rc = sort_segments(ctx, glists.as<Seg>(), (int64_t)G, hg, okey, gb + ybits, out, d_stats);
    if (rc) return rc;
    if (hg[kLarge] > 0) {
        const int nbig = hg[kLarge];
        const Seg *big = glists.as<Seg>() + kLarge * (size_t)G;
        DevBuf blen, bdst, tk, tk2, tv, tv2;
        HY_HIP(blen.alloc(4 * (size_t)(nbig + 1), st));
        HY_HIP(bdst.alloc(8 * (size_t)(nbig + 1), st));
        hipLaunchKernelGGL(seg_len_kernel, dim3((unsigned)cdiv(nbig, 256)), dim3(256), 0, st, big, nbig, blen.as<uint32_t>());
        HY_CHECK_LAUNCH("seg_len_kernel");
        int64_t NB = 0;
        rc = exclusive_scan_u32_i64(ctx, blen.as<uint32_t>(), bdst.as<int64_t>(), nbig, &NB);
        if (rc) return rc;
        HY_HIP(tk.alloc(8 * (size_t)NB, st));
        HY_HIP(tk2.alloc(8 * (size_t)NB, st));
        HY_HIP(tv.alloc(4 * (size_t)NB, st));
        HY_HIP(tv2.alloc(4 * (size_t)NB, st));
        hipLaunchKernelGGL(big_gather_kernel, dim3((unsigned)nbig), dim3(256), 0, st, big, bdst.as<int64_t>(), gb, ybits, okey,
                           tk.as<uint64_t>(), tv.as<uint32_t>());
        HY_CHECK_LAUNCH("big_gather_kernel");
        const int end_bit = gb + bits_of(nbig);
        HY_ARG(end_bit <= 64, "grouped_anchor_sort: group rank and key bits exceed 64");
        uint64_t *kk = tk.as<uint64_t>(), *kka = tk2.as<uint64_t>();
        uint32_t *vv = tv.as<uint32_t>(), *vva = tv2.as<uint32_t>();
        rc = radix_sort_pairs(ctx, kk, kka, vv, vva, NB, 0, end_bit);
        if (rc) return rc;
        hipLaunchKernelGGL(big_put_kernel, dim3((unsigned)nbig), dim3(256), 0, st, big, bdst.as<int64_t>(), gb, ybits, okey,
                           kk, vv, out);
        HY_CHECK_LAUNCH("big_put_kernel");
    }
    return HYMET_OK;
}

}  // namespace mm
}  // namespace hymet

extern "C" int hymet_mm_anchor_sort(hymet_ctx *ctx, const uint64_t *h_key, const uint32_t *h_val, int64_t n,
                                    const int64_t *h_qoff, int32_t n_q, int32_t rb, int32_t pb, uint64_t yhi,
                                    int64_t max_qlen, uint64_t *h_ax, uint64_t *h_ay, uint32_t *h_ax32, uint32_t *h_hb,
                                    int64_t *h_stats) {
    using hymet::mm::DevBuf;
    HY_ARG(ctx && h_key && h_val && h_qoff && h_ax && h_ay && h_ax32 && h_hb, "hymet_mm_anchor_sort: null argument");
    HY_ARG(n > 0 && n < INT32_MAX && n_q > 0, "hymet_mm_anchor_sort: n or n_q out of range");
    HY_ARG(rb >= 0 && pb >= 1 && rb + pb < 63 && max_qlen >= 0, "hymet_mm_anchor_sort: key layout out of range");
    HY_ARG(h_qoff[0] == 0 && h_qoff[n_q] == n, "hymet_mm_anchor_sort: query offsets do not span the anchors");
    for (int32_t q = 0; q < n_q; q++) HY_ARG(h_qoff[q] <= h_qoff[q + 1], "hymet_mm_anchor_sort: query offsets not rising");
    HY_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // no word for this layout: the caller's fallback code, as from the stage itself
    const int ybits = hymet::mm::anchor_word_ybits(rb, pb, max_qlen);
    if (ybits == 0) return 1;
    // a y beyond its field would run into the word's position bits
    for (int64_t i = 0; i < n; i++)
        HY_ARG(((uint64_t)h_val[i] >> ybits) == 0, "hymet_mm_anchor_sort: a y value does not fit the bits of max_qlen");
    DevBuf key, val, qoff, word, okey, ax, ay, ax32, hb, stats;
    const size_t hb_bytes = hymet::mm::head_bits_bytes(n);
    HY_HIP(key.alloc(8 * (size_t)n, st));
    HY_HIP(val.alloc(4 * (size_t)n, st));
    HY_HIP(qoff.alloc(8 * (size_t)(n_q + 1), st));
    HY_HIP(word.alloc(8 * (size_t)n, st));
    HY_HIP(okey.alloc(8 * (size_t)n, st));
    HY_HIP(ax.alloc(8 * (size_t)n, st));
    HY_HIP(ay.alloc(4 * (size_t)n, st));
    HY_HIP(ax32.alloc(4 * (size_t)n, st));
    HY_HIP(hb.alloc(hb_bytes, st));
    HY_HIP(stats.alloc(8 * hymet::mm::kStats, st));
    HY_HIP(hipMemcpyAsync(key.p, h_key, 8 * (size_t)n, hipMemcpyHostToDevice, st));
    HY_HIP(hipMemcpyAsync(val.p, h_val, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    HY_HIP(hipMemcpyAsync(qoff.p, h_qoff, 8 * (size_t)(n_q + 1), hipMemcpyHostToDevice, st));
    HY_HIP(hipMemsetAsync(stats.p, 0, 8 * hymet::mm::kStats, st));
    hipLaunchKernelGGL(hymet::mm::pack_words_kernel, dim3((unsigned)hymet::cdiv(n, 256)), dim3(256), 0, st, key.as<uint64_t>(),
                       val.as<uint32_t>(), n, 1 + rb + pb, ybits, word.as<uint64_t>());
    HY_CHECK_LAUNCH("pack_words_kernel");
    const int rc = hymet::mm::grouped_anchor_sort(ctx, word.as<uint64_t>(), n, qoff.as<int64_t>(), n_q, rb, pb, max_qlen,
                                                  okey.as<uint64_t>(), ax.as<uint64_t>(), ay.as<uint32_t>(),
                                                  hb.as<uint32_t>(), ax32.as<uint32_t>(),
                                                  h_stats ? stats.as<unsigned long long>() : nullptr);
    if (rc) {
        HY_HIP(hipStreamSynchronize(st));  // the uploads read the caller's arrays
        return rc;
    }
    HY_HIP(hipMemcpyAsync(h_ax, ax.p, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
    std::vector<uint32_t> y32((size_t)n);  // y is 32-bit on the device: widened with the span for the caller
    HY_HIP(hipMemcpyAsync(y32.data(), ay.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HY_HIP(hipMemcpyAsync(h_ax32, ax32.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HY_HIP(hipMemcpyAsync(h_hb, hb.p, 4 * (size_t)((n + 31) / 32), hipMemcpyDeviceToHost, st));
    if (h_stats) HY_HIP(hipMemcpyAsync(h_stats, stats.p, 8 * hymet::mm::kStats, hipMemcpyDeviceToHost, st));
    HY_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; i++) h_ay[i] = yhi << 32 | y32[(size_t)i];
    return HYMET_OK;
}

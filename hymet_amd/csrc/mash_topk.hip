// Nearest references of Mash `dist` on MI355X: the K best entries of every row of a dist result,
// nearest first (`cli dist --top K`; DESIGN.md §3 "Nearest (top-K)").  The row is either a row of
// the dense block hymet_mash_dist writes or a row of the CSR hymet_mash_dist_select and
// hymet_mash_dist_sparse write; an entry is the packed common << 16 | denom.
//
// Order.  Nearest first by the exact rational common / denom, descending, 0 / 0 counting as 1;
// equal rationals by reference index, ascending.  One 64-bit key gives it:
//   rank = 2^31 - floor(common * 2^31 / denom)   (0 for denom == 0),   key = rank << 32 | position
// Two different fractions with denominators up to 2^14 differ by at least 2^-28, so their scaled
// values differ by at least 8 and the floors keep the order strictly; equal fractions give equal
// ranks.  The position (the reference index in a dense row, the entry's place in a CSR row, whose
// reference indices ascend) makes every key of a row distinct: the K smallest keys are one set,
// whatever the chunking and the schedule.  No float arithmetic, no global atomics.
//
// Kernels
//   topk_chunk<CSR>: one 256-thread workgroup per (row, chunk of the row's entries).  It reads the
//                    packed values with 16-byte loads between the chunk's first and last 16-byte
//                    boundary (single entries before and after), drops what the optional filter
//                    table or the contract (denom <= s, common <= denom) excludes and keeps the K
//                    smallest keys in LDS.  A row with one chunk writes its result, else the chunk
//                    writes its keys to scratch.
//   topk_merge<CSR>: one workgroup per row; a row with several chunks streams their keys through
//                    the same LDS set and writes the result.
//
// The LDS set (all dynamic, 16-byte aligned): a 64-byte header {n, full, cut} and buf[cap] of
// uint64, cap = the power of two >= K + 1,024.  buf[0, n) holds the kept keys of the last
// compaction (sorted, at most K) followed by the keys staged since.  A key is staged when the set
// is not yet full or the key is below the cut (= kept[K - 1]); one wave ballot and one LDS atomic
// per wave reserve the slots.  Before a step that could stage more than the free room the
// workgroup compacts: bitonic sort of buf[0, n), truncate to K, set the cut.  After a compaction
// n <= K and cap - K >= one step's entries, so a staged key always has a slot.  The cut every
// thread holds is read after the room check of its step, and a stale (higher) cut would only
// stage more.  The chunk kernel tests an entry against the cut's own (common, denom, position)
// by cross-multiplication and divides only in a wave that stages something: the test is the key
// comparison exactly, because equal ranks mean equal fractions.
#include "mash_rank.hpp"
#include "mm_common.hpp"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr int kVec = 4;                      // entries per 16-byte load
constexpr int kStep = kThreads * kVec;       // entries one step can stage
constexpr int kHdrBytes = 64;
constexpr int kMaxK = 1024;                  // cap 2,048: 16 KiB + header per workgroup
constexpr int kMaxS = 16384;                 // hymet_sketch_max_size()
constexpr int kDefaultChunk = 16384;         // fewest entries of a chunk (64 KiB of a row)

// header words (uint32): [0] n, [1] full, [2..3] cut (uint64)
struct TopK {
    uint32_t *hdr;
    uint64_t *buf;
    int K, cap;
    __device__ __forceinline__ uint64_t &cut() const { return *reinterpret_cast<uint64_t *>(hdr + 2); }
};

inline int topk_cap(int K) {
    int p = 1;
    while (p < K + kStep) p <<= 1;
    return p;
}
inline size_t topk_lds(int K) { return (size_t)kHdrBytes + 8 * (size_t)topk_cap(K); }

__device__ __forceinline__ void topk_init(const TopK &T) {
    if (threadIdx.x == 0) {
        T.hdr[0] = 0;
        T.hdr[1] = 0;
        T.cut() = ~0ull;
    }
    __syncthreads();
}

// the key of entry (common c, denom d) at position pos: c <= d <= 2^14 (mash_rank.hpp)
__device__ __forceinline__ uint64_t topk_key(uint32_t c, uint32_t d, uint32_t pos) {
    return hymet::mash_rank_key(c, d, pos);
}

// Stage key for every lane of the ballot m (the lanes with acc set, m != 0).  Every lane of the
// wave calls it (converged).
__device__ __forceinline__ void topk_stage(const TopK &T, uint64_t key, bool acc, uint64_t m) {
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&T.hdr[0], (uint32_t)__popcll(m));
    base = __shfl(base, leader, 64);
    if (acc) T.buf[base + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = key;
}

__device__ __forceinline__ void cmp_swap(uint64_t *buf, int i, int j) {
    const uint64_t a = buf[i], b = buf[j];
    if (a > b) {
        buf[i] = b;
        buf[j] = a;
    }
}

// sort + truncate to K; every thread of the workgroup calls it
__device__ void topk_compact(const TopK &T) {
    __syncthreads();  // every staged key is in buf, every reader of the old state is done
    const int n = (int)T.hdr[0];
    uint64_t *buf = T.buf;
    int P = 1;
    while (P < n) P <<= 1;
    // Bitonic sort whose compare-exchanges all put the smaller value at the lower index (each
    // merge starts with a mirrored step).  Indices >= n stand for +inf: a pair whose upper
    // index is >= n never swaps, so it is skipped, and no +inf ever has to move below n.
    for (int lk = 1; (1 << lk) <= P; lk++) {  // merge sorted blocks of k / 2 into blocks of k = 2^lk
        const int k = 1 << lk, hk = k >> 1;
        for (int t = threadIdx.x; t < (P >> 1); t += kThreads) {
            const int base = (t >> (lk - 1)) << lk, off = t & (hk - 1);
            const int i = base + off, j = base + k - 1 - off;
            if (j < n) cmp_swap(buf, i, j);
        }
        __syncthreads();
        for (int lj = lk - 2; lj >= 0; lj--) {  // half-cleaners at distance jj = 2^lj
            const int jj = 1 << lj;
            for (int t = threadIdx.x; t < (P >> 1); t += kThreads) {
                const int i = ((t >> lj) << (lj + 1)) + (t & (jj - 1)), j = i + jj;
                if (j < n) cmp_swap(buf, i, j);
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0 && n >= T.K) {  // the keys are distinct: nothing to drop but the tail
        T.hdr[0] = (uint32_t)T.K;
        T.hdr[1] = 1;
        T.cut() = buf[T.K - 1];
    }
    __syncthreads();
}

// Before a step that stages at most `step` keys: compact unless there is room for all of them.
// Two barriers: every thread must read n before any thread stages again.
__device__ __forceinline__ void topk_room(const TopK &T, int step, bool &full, uint64_t &cut) {
    __syncthreads();
    const uint32_t n = T.hdr[0];
    __syncthreads();
    if (n + (uint32_t)step > (uint32_t)T.cap) topk_compact(T);  // workgroup-uniform
    full = T.hdr[1] != 0;
    cut = T.cut();
}

// A row and how it is cut into chunks.  vals: the row's packed values; len: its entries (below
// 2^31); base: the row's first entry in the CSR arrays (0 for a dense row).  A row has
// nc = min(nch, len / min_chunk) chunks (at least 1) of clen entries, the last one shorter: no
// chunk of a row with several holds fewer than min_chunk entries.
struct Row {
    const uint32_t *vals;
    int64_t base;
    int len, nc, clen;
};

template <bool CSR>
__device__ __forceinline__ Row topk_row(const uint32_t *__restrict__ vals, int64_t n_ref,
                                        const int64_t *__restrict__ row_off, int64_t row, int nch, int min_chunk) {
    Row R;
    if (CSR) {
        R.base = row_off[row];
        R.len = (int)max((int64_t)0, min(row_off[row + 1] - R.base, (int64_t)0x7fffffff));
        R.vals = vals + R.base;
    } else {
        R.base = 0;
        R.len = (int)n_ref;
        R.vals = vals + (size_t)row * (size_t)n_ref;
    }
    R.nc = max(1, min(nch, R.len / min_chunk));
    R.clen = (R.len + R.nc - 1) / R.nc;
    R.nc = R.clen > 0 ? (R.len + R.clen - 1) / R.clen : 1;
    return R;
}

// the sorted keys of the set as the row's result: reference index, packed value, count
template <bool CSR>
__device__ __forceinline__ void topk_write(const TopK &T, const Row &R, const int32_t *__restrict__ ref_idx, int64_t row,
                                           int32_t *__restrict__ out_idx, uint32_t *__restrict__ out_val,
                                           int32_t *__restrict__ out_cnt) {
    const int n = (int)T.hdr[0];  // at most K after the final compaction
    const size_t o = (size_t)row * (size_t)T.K;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const uint32_t pos = (uint32_t)T.buf[i];  // below R.len
        out_idx[o + i] = CSR ? ref_idx[R.base + pos] : (int32_t)pos;
        out_val[o + i] = R.vals[pos];
    }
    if (threadIdx.x == 0) out_cnt[row] = n;
}

// grid: n_rows * nch workgroups; workgroup b = (row b / nch, chunk b % nch); the chunks a short
// row does not have leave at once
template <bool CSR>
__global__ __launch_bounds__(kThreads) void topk_chunk_kernel(const uint32_t *__restrict__ vals, int64_t n_ref,
                                                              const int64_t *__restrict__ row_off,
                                                              const int32_t *__restrict__ ref_idx,
                                                              const uint16_t *__restrict__ minc, int s, int K, int cap,
                                                              int nch, int min_chunk, uint64_t *__restrict__ part,
                                                              int32_t *__restrict__ part_n, int32_t *__restrict__ out_idx,
                                                              uint32_t *__restrict__ out_val,
                                                              int32_t *__restrict__ out_cnt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const TopK T{reinterpret_cast<uint32_t *>(smem), reinterpret_cast<uint64_t *>(smem + kHdrBytes), K, cap};
    const int64_t row = blockIdx.x / (unsigned)nch;
    const int ch = (int)(blockIdx.x % (unsigned)nch);
    const Row R = topk_row<CSR>(vals, n_ref, row_off, row, nch, min_chunk);
    if (ch >= R.nc) return;  // workgroup-uniform, before the first barrier
    topk_init(T);
    const int e0 = (int)min((int64_t)ch * R.clen, (int64_t)R.len), e1 = (int)min((int64_t)e0 + R.clen, (int64_t)R.len);
    const uint32_t *p = R.vals + e0;
    const int n = e1 - e0;
    const int head = min(n, (int)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2));
    const int nvec = (n - head) >> 2;
    const int tail0 = head + 4 * nvec;  // fewer than 4 entries follow

    bool full = false;
    uint64_t cut = ~0ull, seen = ~0ull;
    uint32_t cut_c = 0, cut_d = 1, cut_pos = 0;  // the cut's entry, 0 / 0 as 1 / 1
    auto room = [&](int step) {
        topk_room(T, step, full, cut);
        if (full && cut != seen) {  // workgroup-uniform
            seen = cut;
            cut_pos = (uint32_t)cut;
            const uint32_t v = R.vals[cut_pos];
            cut_d = v & 0xffffu;
            cut_c = cut_d ? v >> 16 : 1u;
            cut_d = cut_d ? cut_d : 1u;
        }
    };
    // offer entry e of the chunk (position e0 + e of the row); every lane of the wave calls it
    auto entry = [&](int e, uint32_t v, bool in) {
        const uint32_t d = v & 0xffffu, c = v >> 16;
        bool ok = in && d <= (uint32_t)s && c <= d;
        if (ok && minc) ok = c >= (uint32_t)minc[d];
        const uint32_t pos = (uint32_t)(e0 + e);
        // c / d against the cut's: products below 2^28
        const uint32_t a = (d ? c : 1u) * cut_d, b = cut_c * (d ? d : 1u);
        const bool acc = ok && (!full || a > b || (a == b && pos < cut_pos));
        const uint64_t m = __ballot(acc);
        if (m == 0) return;  // wave-uniform
        topk_stage(T, topk_key(c, d, pos), acc, m);
    };

    // the entries before the first and after the last 16-byte boundary: at most 3 + 3, in two waves
    room(kStep);
    {
        const int t = threadIdx.x;
        const bool h = t < head, tl = t >= 64 && tail0 + (t - 64) < n;
        const int e = h ? t : tail0 + (t - 64);
        entry(e, h || tl ? p[e] : 0u, h || tl);
    }
    const uint4 *pv = reinterpret_cast<const uint4 *>(p + head);
    for (int i0 = 0; i0 < nvec; i0 += kThreads) {  // workgroup-uniform trip count
        room(kStep);
        const int i = i0 + (int)threadIdx.x;
        const bool in = i < nvec;
        const uint4 v = in ? pv[i] : make_uint4(0, 0, 0, 0);
        const int e = head + 4 * i;
        entry(e, v.x, in);
        entry(e + 1, v.y, in);
        entry(e + 2, v.z, in);
        entry(e + 3, v.w, in);
    }
    topk_compact(T);
    if (R.nc == 1) {
        topk_write<CSR>(T, R, ref_idx, row, out_idx, out_val, out_cnt);
    } else {
        const int kept = (int)T.hdr[0];
        uint64_t *o = part + (size_t)blockIdx.x * (size_t)K;
        for (int i = threadIdx.x; i < kept; i += kThreads) o[i] = T.buf[i];
        if (threadIdx.x == 0) part_n[blockIdx.x] = kept;
    }
}

// grid: n_rows workgroups; a row with one chunk was written by its chunk
template <bool CSR>
__global__ __launch_bounds__(kThreads) void topk_merge_kernel(const uint32_t *__restrict__ vals, int64_t n_ref,
                                                              const int64_t *__restrict__ row_off,
                                                              const int32_t *__restrict__ ref_idx, int K, int cap, int nch,
                                                              int min_chunk, const uint64_t *__restrict__ part,
                                                              const int32_t *__restrict__ part_n,
                                                              int32_t *__restrict__ out_idx, uint32_t *__restrict__ out_val,
                                                              int32_t *__restrict__ out_cnt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const TopK T{reinterpret_cast<uint32_t *>(smem), reinterpret_cast<uint64_t *>(smem + kHdrBytes), K, cap};
    const int64_t row = blockIdx.x;
    const Row R = topk_row<CSR>(vals, n_ref, row_off, row, nch, min_chunk);
    if (R.nc <= 1) return;  // workgroup-uniform, before the first barrier
    topk_init(T);
    bool full = false;
    uint64_t cut = ~0ull;
    for (int ch = 0; ch < R.nc; ch++) {
        const size_t b = (size_t)row * (size_t)nch + (size_t)ch;
        const uint64_t *keys = part + b * (size_t)K;
        const int n = min(part_n[b], K);
        for (int i0 = 0; i0 < n; i0 += kThreads) {
            topk_room(T, kThreads, full, cut);
            const int i = i0 + (int)threadIdx.x;
            const bool ok = i < n;
            const uint64_t key = ok ? keys[i] : 0;
            const bool acc = ok && (!full || key < cut);
            const uint64_t m = __ballot(acc);
            if (m != 0) topk_stage(T, key, acc, m);  // wave-uniform
        }
    }
    topk_compact(T);
    topk_write<CSR>(T, R, ref_idx, row, out_idx, out_val, out_cnt);
}

// fewest entries per chunk; 0: the default (hymet_mash_topk_tune)
int &chunk_setting() {
    static int c = 0;
    return c;
}
int min_chunk() { return chunk_setting() > 0 ? chunk_setting() : kDefaultChunk; }

// both kernels over n_rows rows cut into at most nch chunks each
template <bool CSR>
int launch_topk(hymet_ctx *ctx, const char *scope, double alg_bytes, const uint32_t *vals, int64_t n_rows, int64_t n_ref,
                const int64_t *row_off, const int32_t *ref_idx, const uint16_t *minc, int s, int K, int nch, int32_t *d_idx,
                uint32_t *d_val, int32_t *d_cnt) {
    hipStream_t st = ctx->stream;
    hymet::mm::DevBuf part, part_n;
    if (nch > 1) {
        HY_HIP(part.alloc(8 * (size_t)n_rows * (size_t)nch * (size_t)K, st));
        HY_HIP(part_n.alloc(4 * (size_t)n_rows * (size_t)nch, st));
    }
    const int cap = topk_cap(K), mc = min_chunk();
    const size_t lds = topk_lds(K);
    hymet::ProfScope _ps(ctx, scope, alg_bytes);
    hipLaunchKernelGGL(topk_chunk_kernel<CSR>, dim3((unsigned)(n_rows * nch)), dim3(kThreads), lds, st, vals, n_ref, row_off,
                       ref_idx, minc, s, K, cap, nch, mc, part.as<uint64_t>(), part_n.as<int32_t>(), d_idx, d_val, d_cnt);
    HY_CHECK_LAUNCH("topk_chunk_kernel");
    if (nch > 1) {
        hipLaunchKernelGGL(topk_merge_kernel<CSR>, dim3((unsigned)n_rows), dim3(kThreads), lds, st, vals, n_ref, row_off,
                           ref_idx, K, cap, nch, mc, part.as<uint64_t>(), part_n.as<int32_t>(), d_idx, d_val, d_cnt);
        HY_CHECK_LAUNCH("topk_merge_kernel");
    }
    return HYMET_OK;
}

// chunks per row that fill the card when the rows alone do not: 8 workgroups per CU
int64_t chunks_for(const hymet_ctx *ctx, int64_t n_rows) { return std::max<int64_t>(1, (int64_t)ctx->n_cu * 8 / n_rows); }

}  // namespace

extern "C" {

int32_t hymet_mash_topk_max(void) { return kMaxK; }

int hymet_mash_topk_tune(int chunk_entries) {
    HY_ARG(chunk_entries >= -1 && chunk_entries <= (1 << 30), "hymet_mash_topk_tune: chunk_entries in -1..2^30");
    if (chunk_entries >= 0) chunk_setting() = chunk_entries;
    return HYMET_OK;
}

int hymet_mash_dist_topk(hymet_ctx *ctx, const uint32_t *d_block, int64_t n_rows, int64_t n_ref,
                         const uint16_t *d_min_common, int32_t s, int32_t K, int32_t *d_idx, uint32_t *d_val,
                         int32_t *d_cnt) {
    HY_ARG(ctx, "hymet_mash_dist_topk: null context");
    HY_ARG(K >= 1 && K <= kMaxK, "hymet_mash_dist_topk: K must be in 1.." + std::to_string(kMaxK));
    HY_ARG(s >= 1 && s <= kMaxS, "hymet_mash_dist_topk: sketch size must be in 1.." + std::to_string(kMaxS));
    HY_ARG(n_rows >= 0 && n_rows < (1ll << 31) && n_ref >= 0 && n_ref < (1ll << 31),
           "hymet_mash_dist_topk: count out of range");
    HY_HIP(hipSetDevice(ctx->device));
    if (n_rows == 0) return HYMET_OK;
    HY_ARG(d_cnt, "hymet_mash_dist_topk: null count output");
    if (n_ref == 0) {
        HY_HIP(hipMemsetAsync(d_cnt, 0, 4 * (size_t)n_rows, ctx->stream));
        return HYMET_OK;
    }
    HY_ARG(d_block && d_idx && d_val, "hymet_mash_dist_topk: null argument");
    HY_ARG((reinterpret_cast<uintptr_t>(d_block) & 3) == 0, "hymet_mash_dist_topk: block not 4-byte aligned");
    // every row has n_ref entries: the chunks that exist are known here
    const int nch = (int)std::max<int64_t>(1, std::min(chunks_for(ctx, n_rows), n_ref / min_chunk()));
    HY_ARG(n_rows < (1ll << 31) / nch, "hymet_mash_dist_topk: too many rows in one call");
    return launch_topk<false>(ctx, "mash_dist_topk", (4.0 * (double)n_ref + 12.0 * K) * (double)n_rows, d_block, n_rows, n_ref,
                              nullptr, nullptr, d_min_common, (int)s, (int)K, nch, d_idx, d_val, d_cnt);
}

int hymet_mash_topk_edges(hymet_ctx *ctx, const int64_t *d_row_off, int64_t n_rows, const int32_t *d_ref_idx,
                          const uint32_t *d_val_in, int32_t s, int32_t K, int32_t *d_idx, uint32_t *d_val,
                          int32_t *d_cnt) {
    HY_ARG(ctx, "hymet_mash_topk_edges: null context");
    HY_ARG(K >= 1 && K <= kMaxK, "hymet_mash_topk_edges: K must be in 1.." + std::to_string(kMaxK));
    HY_ARG(s >= 1 && s <= kMaxS, "hymet_mash_topk_edges: sketch size must be in 1.." + std::to_string(kMaxS));
    HY_ARG(n_rows >= 0 && n_rows < (1ll << 31), "hymet_mash_topk_edges: count out of range");
    HY_HIP(hipSetDevice(ctx->device));
    if (n_rows == 0) return HYMET_OK;
    HY_ARG(d_row_off && d_ref_idx && d_val_in && d_idx && d_val && d_cnt, "hymet_mash_topk_edges: null argument");
    HY_ARG((reinterpret_cast<uintptr_t>(d_val_in) & 3) == 0, "hymet_mash_topk_edges: values not 4-byte aligned");
    // The row lengths stay on the device: every row is given the chunks a long one would take (at
    // most 64), and the workgroups of the chunks a row does not have leave at once.
    const int nch = (int)std::min<int64_t>(64, chunks_for(ctx, n_rows));
    // the entries are not known here: 12 K bytes written and two offsets read per row
    return launch_topk<true>(ctx, "mash_topk_edges", (12.0 * K + 16.0) * (double)n_rows, d_val_in, n_rows, 0, d_row_off,
                             d_ref_idx, nullptr, (int)s, (int)K, nch, d_idx, d_val, d_cnt);
}

}  // extern "C"

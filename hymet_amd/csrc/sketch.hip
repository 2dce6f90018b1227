// Mash `sketch` on MI355X: bottom-s MinHash sketches of a whole batch of references in one
// pass over the packed pool (the DB-build side of scripts/mash.sh).
//
// Work unit: a chunk = (sketch id, [pos_begin, pos_end)) of k-mer START positions in pool
// coordinates.  A chunk belongs to one sketch and may span several of its records (the pool's
// 'N' separators invalidate every k-mer that crosses records).  One workgroup = one chunk.
//
// Kernels
//   sketch_chunk<K>: each thread rolls over 64-position tiles of the chunk exactly as
//                    screen_count<K> does (same strand rule, invalid-base handling and K-1 base
//                    warm-up per tile) and offers every hash to the workgroup's exact running
//                    bottom-s set in LDS.  A chunk that is its sketch's only one writes the
//                    final row, else a partial row in scratch.
//   sketch_merge   : one workgroup per sketch with several chunks: streams its partial rows
//                    through the same LDS set and writes the final row.
//
// The LDS set (all in the dynamic region, Guideline 17): a 64-byte header {n, full, cut, scan
// words} and buf[cap] of uint64: buf[0, n) holds the kept hashes of the last compaction (sorted,
// distinct, at most s) followed by the hashes staged since.  A hash is staged when the set is
// not yet full or the hash is below the cut (= kept[s-1]); one wave ballot and one LDS atomic
// per wave reserve the slots.  The cut a thread uses may be stale (too high): that only stages
// more, it never loses a hash.  Before a step that could stage more than the free room
// (cap - n < the step's hashes) the workgroup compacts: in-place bitonic sort of buf[0, n) with
// virtual +inf padding, drop duplicates, truncate to s, update the cut (oracle/mash_oracle.c's
// bottom_offer / bottom_compact).  After a compaction n <= s and cap - s >= one step's hashes,
// so a staged hash always has a slot.  The result is a set written ascending: it depends on
// neither the chunking nor the schedule.  No float arithmetic, no global atomics.
#include "common.hpp"
#include "mash_hash.hpp"

#include <algorithm>
#include <numeric>

namespace {

using namespace hymet::mash;

constexpr int kThreads = 256;
constexpr int kTile = 64;                 // k-mer starts per thread and round (the screen's tile)
constexpr int kSub = 8;                   // starts per thread between two room checks
constexpr int kStage = kThreads * kSub;   // hashes one step can stage
constexpr int kHdrBytes = 64;
constexpr int kMaxSketch = 16384;         // (16384 + 2048) * 8 + 64 B = 144 KiB of the CU's 160 KiB

// header words (uint32): [0] n, [1] full, [2..3] cut (uint64), [4..7] per-wave scan counts
struct Bottom {
    uint32_t *hdr;
    uint64_t *buf;
    int s, cap;
    __device__ __forceinline__ uint64_t &cut() const { return *reinterpret_cast<uint64_t *>(hdr + 2); }
};

// capacity of buf for sketch size s: s kept + one step of staging, rounded up to a power of two
// (the sort works on the next power of two anyway) while that stays under the largest layout
inline int bottom_cap(int s) {
    const int need = s + kStage;
    int p = 1;
    while (p < need) p <<= 1;
    return p <= kMaxSketch ? p : need;
}
inline size_t bottom_lds(int s) { return (size_t)kHdrBytes + 8 * (size_t)bottom_cap(s); }

__device__ __forceinline__ void bottom_init(const Bottom &B) {
    if (threadIdx.x == 0) {
        B.hdr[0] = 0;
        B.hdr[1] = 0;
        B.cut() = ~0ull;
    }
    __syncthreads();
}

// Stage h for every lane with acc set.  Every lane of the wave calls it (converged).
__device__ __forceinline__ void bottom_offer(const Bottom &B, uint64_t h, bool acc) {
    const uint64_t m = __ballot(acc);
    if (m == 0) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&B.hdr[0], (uint32_t)__popcll(m));
    base = __shfl(base, leader, 64);
    if (acc) B.buf[base + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = h;
}

__device__ __forceinline__ void cmp_swap(uint64_t *buf, int i, int j) {
    const uint64_t a = buf[i], b = buf[j];
    if (a > b) {
        buf[i] = b;
        buf[j] = a;
    }
}

// sort + unique + truncate to s; every thread of the workgroup calls it
__device__ void bottom_compact(const Bottom &B) {
    __syncthreads();  // every staged hash is in buf, every reader of the old state is done
    const int n = (int)B.hdr[0];
    uint64_t *buf = B.buf;
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
    // Keep the first of each run of equal values, 256 at a time: flag, scan (ballots + the
    // waves' counts), read to a register, barrier, write.  An element moves to an index <= its
    // own, so a write never lands on a value of a later tile.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t kept = 0;      // distinct values so far (workgroup-uniform)
    uint64_t carry = 0;     // the value before this tile
    for (int t0 = 0; t0 < n && kept < (uint32_t)B.s; t0 += kThreads) {
        const int idx = t0 + (int)threadIdx.x;
        uint64_t v = 0;
        bool flag = false;
        if (idx < n) {
            v = buf[idx];
            const uint64_t prev = threadIdx.x == 0 ? carry : buf[idx - 1];
            flag = idx == 0 || v != prev;
        }
        const uint64_t last = buf[min(t0 + kThreads, n) - 1];
        const uint64_t m = __ballot(flag);
        if (lane == 0) B.hdr[4 + wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; w++) {
            const uint32_t c = B.hdr[4 + w];
            before += w < wave ? c : 0;
            total += c;
        }
        const uint32_t pos = kept + before + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (flag && pos < (uint32_t)B.s) buf[pos] = v;
        kept += total;
        carry = last;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (kept >= (uint32_t)B.s) {
            B.hdr[0] = (uint32_t)B.s;
            B.hdr[1] = 1;
            B.cut() = buf[B.s - 1];
        } else {
            B.hdr[0] = kept;
        }
    }
    __syncthreads();
}

// Before a step that stages at most `step` hashes: compact unless there is room for all of them.
// Two barriers: every thread must read n before any thread stages again.
__device__ __forceinline__ void bottom_room(const Bottom &B, int step, bool &full, uint64_t &cut) {
    __syncthreads();
    const uint32_t n = B.hdr[0];
    __syncthreads();
    if (n + (uint32_t)step > (uint32_t)B.cap) bottom_compact(B);  // workgroup-uniform
    full = B.hdr[1] != 0;
    cut = B.cut();
}

// final compaction, then the row and its count
__device__ __forceinline__ void bottom_write(const Bottom &B, uint64_t *out, int32_t *out_n) {
    bottom_compact(B);
    const int n = (int)B.hdr[0];
    for (int i = threadIdx.x; i < n; i += kThreads) out[i] = B.buf[i];
    if (threadIdx.x == 0) *out_n = n;
}

struct ChunkDesc {
    int64_t begin, end;  // k-mer start positions, pool coordinates
    uint64_t *out;       // the row this chunk writes (final or partial), s entries
    int32_t *out_n;
};

struct MergeDesc {
    const uint64_t *part;    // the sketch's partial rows, n_part x s
    const int32_t *part_n;
    uint64_t *out;
    int32_t *out_n;
    int64_t n_part;
};

template <int K>
__global__ __launch_bounds__(kThreads) void sketch_chunk_kernel(const uint32_t *__restrict__ w2b,
                                                                const uint32_t *__restrict__ wm,
                                                                const ChunkDesc *__restrict__ chunks, uint32_t seed,
                                                                int s, int cap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Bottom B{reinterpret_cast<uint32_t *>(smem), reinterpret_cast<uint64_t *>(smem + kHdrBytes), s, cap};
    const ChunkDesc c = chunks[blockIdx.x];
    bottom_init(B);
    const int64_t n_rounds = (c.end - c.begin + (int64_t)kThreads * kTile - 1) / ((int64_t)kThreads * kTile);
    bool full = false;
    uint64_t cut = ~0ull;
    for (int64_t r = 0; r < n_rounds; r++) {
        const int64_t p0 = c.begin + (r * kThreads + threadIdx.x) * kTile;  // first k-mer start
        const int64_t p1 = min(p0 + kTile, c.end);                          // one past the last
        KmerRoll<K> roll;
        int run = 0;
        uint32_t cw = 0, mw = 0;
        int64_t i = p0;
        auto step = [&]() {  // take base i into the rolling state
            if (((i & 15) == 0) || i == p0) cw = w2b[i >> 4];
            if (((i & 31) == 0) || i == p0) mw = wm[i >> 5];
            const uint32_t b = (cw >> (2 * (i & 15))) & 3u;
            const uint32_t bad = (mw >> (i & 31)) & 1u;
            run = bad ? 0 : run + 1;
            roll.push(b);
            i++;
        };
        // warm-up: the K - 1 bases before the first k-mer's last (p0 < end <= n_bases - K + 1)
        if (p0 < c.end)
            for (int j = 0; j < K - 1; j++) step();
        for (int sub = 0; sub < kTile / kSub; sub++) {
            bottom_room(B, kStage, full, cut);
#pragma unroll 1
            for (int j = 0; j < kSub; j++) {
                bool ok = p0 + sub * kSub + j < p1;  // this start belongs to the thread's tile
                uint64_t h = 0;
                if (ok) {
                    step();
                    ok = run >= K;  // no invalid base inside the k-mer
                    if (ok) h = roll.hash(seed);
                }
                bottom_offer(B, h, ok && (!full || h < cut));
            }
        }
    }
    bottom_write(B, c.out, c.out_n);
}

__global__ __launch_bounds__(kThreads) void sketch_merge_kernel(const MergeDesc *__restrict__ merges, int s, int cap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Bottom B{reinterpret_cast<uint32_t *>(smem), reinterpret_cast<uint64_t *>(smem + kHdrBytes), s, cap};
    const MergeDesc m = merges[blockIdx.x];
    bottom_init(B);
    bool full = false;
    uint64_t cut = ~0ull;
    for (int64_t p = 0; p < m.n_part; p++) {
        const uint64_t *row = m.part + p * s;
        const int n = m.part_n[p];
        for (int e0 = 0; e0 < n; e0 += kThreads) {
            bottom_room(B, kThreads, full, cut);
            const int idx = e0 + (int)threadIdx.x;
            const bool ok = idx < n;
            const uint64_t h = ok ? row[idx] : 0;
            bottom_offer(B, h, ok && (!full || h < cut));
        }
    }
    bottom_write(B, m.out, m.out_n);
}

struct Scratch {
    void *p = nullptr;
    size_t cls = 0;
    hipStream_t st = nullptr;
    ~Scratch() {
        if (p) hymet::scratch_free(p, st, cls);
    }
    hipError_t alloc(size_t bytes, hipStream_t stream) {
        st = stream;
        return hymet::scratch_alloc(bytes ? bytes : 16, stream, &p, &cls);
    }
};

template <int K>
int launch_chunks(hymet_ctx *ctx, const uint32_t *d_2b, const uint32_t *d_mask, const ChunkDesc *d_chunks,
                  int64_t n_chunks, uint32_t seed, int s, double alg_bytes) {
    const size_t lds = bottom_lds(s);
    if (lds > 64 * 1024)
        HY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&sketch_chunk_kernel<K>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hymet::ProfScope _ps(ctx, "sketch_chunk", alg_bytes);
    hipLaunchKernelGGL(sketch_chunk_kernel<K>, dim3((unsigned)n_chunks), dim3(kThreads), lds, ctx->stream, d_2b, d_mask,
                       d_chunks, seed, s, bottom_cap(s));
    HY_CHECK_LAUNCH("sketch_chunk_kernel");
    return HYMET_OK;
}

}  // namespace

extern "C" {

int64_t hymet_sketch_max_size(void) { return kMaxSketch; }

int hymet_sketch_batch(hymet_ctx *ctx, const uint32_t *d_2b, const uint32_t *d_mask, int64_t n_bases, int k,
                       uint32_t seed, int32_t s, int64_t n_chunks, const int32_t *h_chunk_sketch,
                       const int64_t *h_chunk_begin, const int64_t *h_chunk_end, int32_t n_sketches, uint64_t *d_out,
                       int32_t *d_out_n) {
    HY_ARG(ctx, "hymet_sketch_batch: null context");
    HY_ARG(k >= 1 && k <= 32, "hymet_sketch_batch: k must be in 1..32");
    HY_ARG(s >= 1 && s <= kMaxSketch, "hymet_sketch_batch: sketch size must be in 1.." + std::to_string(kMaxSketch));
    HY_ARG(n_chunks >= 0 && n_sketches >= 0 && n_bases >= 0, "hymet_sketch_batch: negative count");
    HY_ARG(n_chunks < (1ll << 31) - 1, "hymet_sketch_batch: more than 2^31 - 2 chunks");
    if (n_sketches == 0) return HYMET_OK;
    HY_ARG(d_out && d_out_n, "hymet_sketch_batch: null output");
    HY_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    HY_HIP(hipMemsetAsync(d_out_n, 0, 4 * (size_t)n_sketches, st));  // sketches with no chunk: empty rows
    if (n_chunks == 0) return HYMET_OK;
    HY_ARG(d_2b && d_mask && h_chunk_sketch && h_chunk_begin && h_chunk_end, "hymet_sketch_batch: null argument");
    // the plan: everything is checked here, before any launch
    const int64_t pos_end = n_bases - k + 1;  // one past the last k-mer start of the pool
    double bases = 0;
    for (int64_t c = 0; c < n_chunks; c++) {
        const int64_t b = h_chunk_begin[c], e = h_chunk_end[c];
        HY_ARG(h_chunk_sketch[c] >= 0 && h_chunk_sketch[c] < n_sketches,
               "hymet_sketch_batch: chunk " + std::to_string(c) + ": sketch id out of range");
        HY_ARG(c == 0 || h_chunk_sketch[c] >= h_chunk_sketch[c - 1],
               "hymet_sketch_batch: chunk " + std::to_string(c) + ": chunks are not sorted by sketch id");
        HY_ARG(b >= 0 && b <= e && e <= pos_end,
               "hymet_sketch_batch: chunk " + std::to_string(c) + ": range outside [0, n_bases - k + 1)");
        bases += (double)(e - b);
    }
    {
        std::vector<int64_t> ord((size_t)n_chunks);
        std::iota(ord.begin(), ord.end(), (int64_t)0);
        std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) {
            return h_chunk_begin[a] != h_chunk_begin[b] ? h_chunk_begin[a] < h_chunk_begin[b]
                                                        : h_chunk_end[a] < h_chunk_end[b];
        });
        int64_t last = -1;  // the non-empty chunk with the largest end so far
        for (int64_t j = 0; j < n_chunks; j++) {
            const int64_t c = ord[j];
            if (h_chunk_begin[c] == h_chunk_end[c]) continue;
            HY_ARG(last < 0 || h_chunk_end[last] <= h_chunk_begin[c],
                   "hymet_sketch_batch: chunks " + std::to_string(last) + " and " + std::to_string(c) + " overlap");
            last = c;
        }
    }
    // a sketch with one chunk is written by that chunk; the others get partial rows in scratch
    int64_t n_part = 0, n_merge = 0;
    for (int64_t c = 0; c < n_chunks;) {
        int64_t e = c + 1;
        while (e < n_chunks && h_chunk_sketch[e] == h_chunk_sketch[c]) e++;
        if (e - c > 1) {
            n_part += e - c;
            n_merge++;
        }
        c = e;
    }
    Scratch d_chunks, d_merges, d_part, d_part_n;
    HY_HIP(d_chunks.alloc(sizeof(ChunkDesc) * (size_t)n_chunks, st));
    if (n_merge) {
        HY_HIP(d_merges.alloc(sizeof(MergeDesc) * (size_t)n_merge, st));
        HY_HIP(d_part.alloc(8 * (size_t)n_part * (size_t)s, st));
        HY_HIP(d_part_n.alloc(4 * (size_t)n_part, st));
    }
    std::vector<ChunkDesc> cd((size_t)n_chunks);
    std::vector<MergeDesc> md((size_t)n_merge);
    uint64_t *part = static_cast<uint64_t *>(d_part.p);
    int32_t *part_n = static_cast<int32_t *>(d_part_n.p);
    int64_t ip = 0, im = 0;
    for (int64_t c = 0; c < n_chunks;) {
        int64_t e = c + 1;
        while (e < n_chunks && h_chunk_sketch[e] == h_chunk_sketch[c]) e++;
        const int64_t r = h_chunk_sketch[c];
        if (e - c == 1) {
            cd[c] = {h_chunk_begin[c], h_chunk_end[c], d_out + r * s, d_out_n + r};
        } else {
            md[im++] = {part + ip * s, part_n + ip, d_out + r * s, d_out_n + r, e - c};
            for (int64_t j = c; j < e; j++, ip++) cd[j] = {h_chunk_begin[j], h_chunk_end[j], part + ip * s, part_n + ip};
        }
        c = e;
    }
    HY_HIP(hipMemcpyAsync(d_chunks.p, cd.data(), sizeof(ChunkDesc) * (size_t)n_chunks, hipMemcpyHostToDevice, st));
    if (n_merge)
        HY_HIP(hipMemcpyAsync(d_merges.p, md.data(), sizeof(MergeDesc) * (size_t)n_merge, hipMemcpyHostToDevice, st));
    const double alg = 0.375 * bases + 8.0 * (double)s * (double)n_chunks;
    const ChunkDesc *dc = static_cast<const ChunkDesc *>(d_chunks.p);
    int rc = HYMET_OK;
    switch (k) {
#define HY_K(KK) \
    case KK: rc = launch_chunks<KK>(ctx, d_2b, d_mask, dc, n_chunks, seed, s, alg); break;
        HY_K(1) HY_K(2) HY_K(3) HY_K(4) HY_K(5) HY_K(6) HY_K(7) HY_K(8)
        HY_K(9) HY_K(10) HY_K(11) HY_K(12) HY_K(13) HY_K(14) HY_K(15) HY_K(16)
        HY_K(17) HY_K(18) HY_K(19) HY_K(20) HY_K(21) HY_K(22) HY_K(23) HY_K(24)
        HY_K(25) HY_K(26) HY_K(27) HY_K(28) HY_K(29) HY_K(30) HY_K(31) HY_K(32)
#undef HY_K
    }
    if (rc) return rc;
    if (n_merge) {
        const size_t lds = bottom_lds(s);
        if (lds > 64 * 1024)
            HY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&sketch_merge_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hymet::ProfScope _ps(ctx, "sketch_merge", 8.0 * (double)s * (double)(n_part + n_merge));
        hipLaunchKernelGGL(sketch_merge_kernel, dim3((unsigned)n_merge), dim3(kThreads), lds, st,
                           static_cast<const MergeDesc *>(d_merges.p), (int)s, bottom_cap(s));
        HY_CHECK_LAUNCH("sketch_merge_kernel");
    }
    return HYMET_OK;
}

}  // extern "C"

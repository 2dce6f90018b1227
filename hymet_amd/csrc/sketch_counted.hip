// Mash `sketch -r -m M` on MI355X: per sketch the s smallest canonical k-mer hashes whose
// multiplicity over all of the sketch's k-mers is at least M, with the multiplicities (read sets:
// a k-mer seen once is almost always a sequencing error; DESIGN.md §3 "Sketch: read sets").
//
// Exact, with no hash threshold supplied or guessed.  The bottom-s DISTINCT set sketch.hip keeps
// per chunk cannot be bent to this: a hash qualifies by its copies summed over all chunks, and
// within one chunk more than s error singletons can lie below it.  Instead every chunk keeps the
// `keep` smallest distinct hashes >= lo WITH their counts, the chunks of a sketch agree on the
// largest hash T up to which all of them are complete, the pairs <= T are summed and selected, and
// if the row is still short the pool is hashed again from lo = T + 1.
//
// Work unit and hashing are sketch.hip's: a chunk = (sketch id, [begin, end)) of k-mer START
// positions in pool coordinates, one 256-thread workgroup per chunk, 64-position tiles per thread
// with a K - 1 base warm-up, KmerRoll<K> (mash_hash.hpp), the same plan checks before any launch.
//
// Kernels of one pass
//   counted_chunk<K>: rolls over the chunk and offers every hash >= lo[sketch] to the counted LDS
//                     set.  The only chunk of its sketch selects from the set itself: it appends
//                     the hashes with count >= M to the row and decides done / the next lo.  Any
//                     other chunk writes its (hash, count) pairs, its cut and whether it filled.
//                     The chunks of a finished sketch leave at once.
//   counted_threshold: per sketch with several chunks, T = the smallest cut among its filled
//                     chunks (all ones when none filled) and, per chunk, how many pairs are <= T.
//   counted_gather  : those pairs into one array, (hash, slot << 32 | count); the library's radix
//                     sort (sort.hpp) orders it by hash, then stably by slot.
//   counted_flag    : the first of every run of equal (slot, hash) sums the run's counts and flags
//                     itself when the sum reaches M; a scan of the flags ranks the qualifiers.
//   counted_append / counted_finish: the qualifiers go to their rows behind what earlier passes
//                     wrote; the sketch is done when its row holds s entries or no chunk filled.
//
// The counted LDS set (all dynamic): a 64-byte header {n, full, cut, scan words, nk}, hashes
// buf[cap] (uint64) and counts cnt[cap] (uint32): 12 B per slot.
// buf[0, nk) holds the kept hashes of the last compaction (sorted, distinct, at most keep) with
// their counts, buf[nk, n) the hashes staged since with count 1 (cap = keep + two steps of staging
// where 160 KiB allow it, at least one: counted_cap).  A hash h is taken when the set
// is not yet full or h <= cut (= kept[keep - 1]) -- `<=`, not the `<` of the distinct-only set:
// the cut hash's own later copies must be counted.  A taken hash that is already in buf[0, nk)
// (binary search) adds 1 to its count in place; only the others are staged, so a deep read set
// does not fill the staging area with copies of what is kept.  Compaction: bitonic sort of the
// pairs by hash, sum each run of equal hashes, truncate to keep, set the cut.  The cut only falls,
// and a stale (higher) cut only stages more, so every hash <= the chunk's final cut was taken at
// every occurrence and never truncated: its count is complete for the chunk.  A set that reached
// keep entries reports "filled" (it may have dropped something); one that did not holds every
// hash >= lo of its chunk.
//
// Counts are 32 bits: a sketch whose chunks span 2^32 positions or more is refused, so no sum can
// wrap.  Integer work only; no global atomics on the result (the rows are written by rank).  The
// result depends on neither the chunking, the schedule nor keep: keep changes the number of passes.
#include "sort.hpp"
#include "mash_hash.hpp"

#include <numeric>

namespace {

using namespace hymet::mash;
using hymet::mm::DevBuf;

constexpr int kThreads = 256;
constexpr int kTile = 64;                 // k-mer starts per thread and round (the screen's tile)
constexpr int kSub = 8;                   // starts per thread between two room checks
constexpr int kStage = kThreads * kSub;   // hashes one step can stage
constexpr int kHdrBytes = 64;
constexpr int kSlotBytes = 12;
constexpr int kMaxCap = (160 * 1024 - kHdrBytes) / kSlotBytes;  // 13,648 slots: the CU's 160 KiB
constexpr int kMaxKeep = kMaxCap - kStage;                      // 11,600
constexpr int kDefaultKeep = 2048;        // 6,144 slots, 72 KiB + header: two workgroups per CU

// header words (uint32): [0] n, [1] full, [2..3] cut (uint64), [4..7] per-wave scan counts, [8] nk
struct Counted {
    uint32_t *hdr;
    uint64_t *buf;
    uint32_t *cnt;
    int keep, cap;
    __device__ __forceinline__ uint64_t &cut() const { return *reinterpret_cast<uint64_t *>(hdr + 2); }
};

// Slots for `keep` kept pairs: one step of staging is needed; a second one lets a full set take
// 2,048 more pairs before it compacts again (with none, every step that stages a single hash
// ends in a sort), as far as the 160 KiB allow.
inline int counted_cap(int keep) { return std::min(kMaxCap, keep + 2 * kStage); }
inline size_t counted_lds(int keep) { return (size_t)kHdrBytes + (size_t)kSlotBytes * (size_t)counted_cap(keep); }

__device__ __forceinline__ Counted counted_set(char *smem, int keep, int cap) {
    return Counted{reinterpret_cast<uint32_t *>(smem), reinterpret_cast<uint64_t *>(smem + kHdrBytes),
                   reinterpret_cast<uint32_t *>(smem + kHdrBytes + 8 * (size_t)cap), keep, cap};
}

__device__ __forceinline__ void counted_init(const Counted &B) {
    if (threadIdx.x == 0) {
        B.hdr[0] = 0;
        B.hdr[1] = 0;
        B.cut() = ~0ull;
        B.hdr[8] = 0;
    }
    __syncthreads();
}

// Take one copy of h for every lane with acc set: count it in place when h is one of the nk kept
// hashes, else stage it with count 1.  Every lane of the wave calls it (converged).
__device__ __forceinline__ void counted_offer(const Counted &B, uint64_t h, bool acc, int nk) {
    if (acc && nk > 0) {
        int lo = 0, hi = nk;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (B.buf[mid] < h) lo = mid + 1;
            else hi = mid;
        }
        if (lo < nk && B.buf[lo] == h) {
            atomicAdd(&B.cnt[lo], 1u);
            acc = false;
        }
    }
    const uint64_t m = __ballot(acc);
    if (m == 0) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&B.hdr[0], (uint32_t)__popcll(m));
    base = __shfl(base, leader, 64);
    if (acc) {
        const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        B.buf[at] = h;
        B.cnt[at] = 1u;
    }
}

__device__ __forceinline__ void cmp_swap(const Counted &B, int i, int j) {
    const uint64_t a = B.buf[i], b = B.buf[j];
    if (a > b) {
        B.buf[i] = b;
        B.buf[j] = a;
        const uint32_t c = B.cnt[i];
        B.cnt[i] = B.cnt[j];
        B.cnt[j] = c;
    }
}

// sort by hash + sum the runs of equal hashes + truncate to keep; every thread of the workgroup
// calls it
__device__ void counted_compact(const Counted &B) {
    __syncthreads();  // every staged hash and in-place count is in, every reader of the old state is done
    const int n = (int)B.hdr[0];
    int P = 1;
    while (P < n) P <<= 1;
    // sketch.hip's bitonic sort: every compare-exchange puts the smaller hash at the lower index,
    // indices >= n stand for +inf and are skipped
    for (int lk = 1; (1 << lk) <= P; lk++) {
        const int k = 1 << lk, hk = k >> 1;
        for (int t = threadIdx.x; t < (P >> 1); t += kThreads) {
            const int base = (t >> (lk - 1)) << lk, off = t & (hk - 1);
            const int i = base + off, j = base + k - 1 - off;
            if (j < n) cmp_swap(B, i, j);
        }
        __syncthreads();
        for (int lj = lk - 2; lj >= 0; lj--) {
            const int jj = 1 << lj;
            for (int t = threadIdx.x; t < (P >> 1); t += kThreads) {
                const int i = ((t >> lj) << (lj + 1)) + (t & (jj - 1)), j = i + jj;
                if (j < n) cmp_swap(B, i, j);
            }
            __syncthreads();
        }
    }
    // The first of each run of equal hashes takes the run's summed count, 256 positions at a time:
    // flag, walk the run (it may reach into later tiles, which nothing has written yet), scan,
    // barrier, write.  An entry moves to an index <= its own.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t kept = 0;      // distinct hashes so far (workgroup-uniform)
    uint64_t carry = 0;     // the hash before this tile
    for (int t0 = 0; t0 < n && kept < (uint32_t)B.keep; t0 += kThreads) {
        const int idx = t0 + (int)threadIdx.x;
        uint64_t v = 0;
        uint32_t sum = 0;
        bool flag = false;
        if (idx < n) {
            v = B.buf[idx];
            const uint64_t prev = threadIdx.x == 0 ? carry : B.buf[idx - 1];
            flag = idx == 0 || v != prev;
            if (flag)
                for (int j = idx; j < n && B.buf[j] == v; j++) sum += B.cnt[j];
        }
        const uint64_t last = B.buf[min(t0 + kThreads, n) - 1];
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
        if (flag && pos < (uint32_t)B.keep) {
            B.buf[pos] = v;
            B.cnt[pos] = sum;
        }
        kept += total;
        carry = last;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (kept >= (uint32_t)B.keep) {
            B.hdr[0] = B.hdr[8] = (uint32_t)B.keep;
            B.hdr[1] = 1;
            B.cut() = B.buf[B.keep - 1];
        } else {
            B.hdr[0] = B.hdr[8] = kept;
        }
    }
    __syncthreads();
}

// Before a step that stages at most kStage hashes: compact unless there is room for all of them.
// Two barriers: every thread must read n before any thread stages again.
__device__ __forceinline__ void counted_room(const Counted &B, bool &full, uint64_t &cut, int &nk) {
    __syncthreads();
    const uint32_t n = B.hdr[0];
    __syncthreads();
    if (n + (uint32_t)kStage > (uint32_t)B.cap) counted_compact(B);  // workgroup-uniform
    full = B.hdr[1] != 0;
    cut = B.cut();
    nk = (int)B.hdr[8];
}

struct CChunk {
    int64_t begin, end;  // k-mer start positions, pool coordinates
    int32_t sketch;
    int32_t part;        // its place in the partial arrays; -1: the only chunk of its sketch
};

struct PartMeta {
    uint64_t cut;
    int32_t n, full;
};

struct MultiDesc {   // a sketch with several chunks: parts [part0, part0 + n_part)
    int32_t sketch, part0, n_part;
};

// the state of every sketch between passes
struct SketchState {
    uint64_t *lo;    // hashes below are dealt with
    int32_t *done;
};

template <int K>
__global__ __launch_bounds__(kThreads) void counted_chunk_kernel(
    const uint32_t *__restrict__ w2b, const uint32_t *__restrict__ wm, const CChunk *__restrict__ chunks, uint32_t seed,
    int s, int keep, int cap, uint32_t min_copies, SketchState st, uint64_t *__restrict__ out, uint32_t *__restrict__ out_count,
    int32_t *__restrict__ out_n, uint64_t *__restrict__ part_h, uint32_t *__restrict__ part_c,
    PartMeta *__restrict__ part_meta) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Counted B = counted_set(smem, keep, cap);
    const CChunk c = chunks[blockIdx.x];
    if (st.done[c.sketch]) return;  // workgroup-uniform, before the first barrier
    const uint64_t lo = st.lo[c.sketch];
    counted_init(B);
    const int64_t n_rounds = (c.end - c.begin + (int64_t)kThreads * kTile - 1) / ((int64_t)kThreads * kTile);
    bool full = false;
    uint64_t cut = ~0ull;
    int nk = 0;
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
            counted_room(B, full, cut, nk);
#pragma unroll 1
            for (int j = 0; j < kSub; j++) {
                bool ok = p0 + sub * kSub + j < p1;  // this start belongs to the thread's tile
                uint64_t h = 0;
                if (ok) {
                    step();
                    ok = run >= K;  // no invalid base inside the k-mer
                    if (ok) h = roll.hash(seed);
                }
                counted_offer(B, h, ok && h >= lo && (!full || h <= cut), nk);
            }
        }
    }
    counted_compact(B);
    const int n = (int)B.hdr[0];
    full = B.hdr[1] != 0;
    cut = B.cut();
    if (c.part >= 0) {
        uint64_t *ph = part_h + (size_t)c.part * (size_t)keep;
        uint32_t *pc = part_c + (size_t)c.part * (size_t)keep;
        for (int i = threadIdx.x; i < n; i += kThreads) {
            ph[i] = B.buf[i];
            pc[i] = B.cnt[i];
        }
        if (threadIdx.x == 0) part_meta[c.part] = PartMeta{cut, n, full ? 1 : 0};
        return;
    }
    // The sketch's only chunk: everything in the set is complete (it is <= the cut, or the set
    // never filled).  Append the hashes with enough copies behind the row's earlier entries.
    const int have = out_n[c.sketch];
    uint64_t *row = out + (size_t)c.sketch * (size_t)s;
    uint32_t *rowc = out_count + (size_t)c.sketch * (size_t)s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t added = 0;  // workgroup-uniform
    for (int t0 = 0; t0 < n && have + (int)added < s; t0 += kThreads) {
        const int idx = t0 + (int)threadIdx.x;
        const bool q = idx < n && B.cnt[idx] >= min_copies;
        const uint64_t m = __ballot(q);
        if (lane == 0) B.hdr[4 + wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; w++) {
            const uint32_t cc = B.hdr[4 + w];
            before += w < wave ? cc : 0;
            total += cc;
        }
        const int64_t pos = (int64_t)have + added + before + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (q && pos < s) {
            row[pos] = B.buf[idx];
            rowc[pos] = B.cnt[idx];
        }
        added += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int n_new = (int)min((int64_t)s, (int64_t)have + added);
        out_n[c.sketch] = n_new;
        st.done[c.sketch] = (n_new >= s || !full || cut == ~0ull) ? 1 : 0;
        st.lo[c.sketch] = cut + 1;
    }
}

// the pairs of part p that are <= T (its hashes ascend)
__device__ __forceinline__ int count_le(const uint64_t *h, int n, uint64_t T) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (h[mid] <= T) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// grid: the sketches with several chunks
__global__ __launch_bounds__(kThreads) void counted_threshold_kernel(const MultiDesc *__restrict__ multi, int keep,
                                                                     SketchState st, const uint64_t *__restrict__ part_h,
                                                                     const PartMeta *__restrict__ part_meta,
                                                                     uint64_t *__restrict__ multi_T,
                                                                     uint32_t *__restrict__ take) {
    __shared__ unsigned long long sT;
    const MultiDesc d = multi[blockIdx.x];
    if (st.done[d.sketch]) {  // workgroup-uniform; its chunks wrote nothing in this pass
        for (int j = threadIdx.x; j < d.n_part; j += kThreads) take[d.part0 + j] = 0;
        return;
    }
    if (threadIdx.x == 0) sT = ~0ull;
    __syncthreads();
    unsigned long long mine = ~0ull;
    for (int j = threadIdx.x; j < d.n_part; j += kThreads) {
        const PartMeta pm = part_meta[d.part0 + j];
        if (pm.full && pm.cut < mine) mine = pm.cut;
    }
    if (mine != ~0ull) atomicMin(&sT, mine);
    __syncthreads();
    const uint64_t T = sT;
    for (int j = threadIdx.x; j < d.n_part; j += kThreads) {
        const int p = d.part0 + j;
        take[p] = (uint32_t)count_le(part_h + (size_t)p * (size_t)keep, part_meta[p].n, T);
    }
    if (threadIdx.x == 0) multi_T[blockIdx.x] = T;
}

// grid: the parts; part p's first take[p] pairs go to [off[p], off[p] + take[p])
__global__ __launch_bounds__(kThreads) void counted_gather_kernel(int keep, const int32_t *__restrict__ part_slot,
                                                                  const uint64_t *__restrict__ part_h,
                                                                  const uint32_t *__restrict__ part_c,
                                                                  const uint32_t *__restrict__ take,
                                                                  const int64_t *__restrict__ off,
                                                                  uint64_t *__restrict__ keys, uint64_t *__restrict__ vals) {
    const int p = blockIdx.x;
    const int n = (int)take[p];
    const int64_t o = off[p];
    const uint64_t slot = (uint64_t)(uint32_t)part_slot[p] << 32;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        keys[o + i] = part_h[(size_t)p * (size_t)keep + i];
        vals[o + i] = slot | part_c[(size_t)p * (size_t)keep + i];
    }
}

// Over the pairs sorted by (slot, hash): the first pair of a run sums the run's counts (a run is
// at most one pair per chunk of the sketch) and flags itself when the sum reaches min_copies.
// flag has n + 1 entries, the last one 0, so that the scan ends with the total.
__global__ __launch_bounds__(kThreads) void counted_flag_kernel(const uint64_t *__restrict__ keys,
                                                                const uint64_t *__restrict__ vals, int64_t n,
                                                                uint32_t min_copies, uint32_t *__restrict__ flag,
                                                                uint32_t *__restrict__ sum) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i > n) return;
    uint32_t f = 0;
    if (i < n) {
        const uint64_t h = keys[i], slot = vals[i] >> 32;
        if (i == 0 || keys[i - 1] != h || (vals[i - 1] >> 32) != slot) {
            uint64_t t = 0;  // below 2^32: a sketch spans fewer than 2^32 positions
            for (int64_t j = i; j < n && keys[j] == h && (vals[j] >> 32) == slot; j++) t += (uint32_t)vals[j];
            const uint32_t c = t > 0xffffffffull ? 0xffffffffu : (uint32_t)t;
            sum[i] = c;
            f = c >= min_copies ? 1u : 0u;
        }
    }
    flag[i] = f;
}

// a flagged pair's rank among its sketch's flagged pairs places it behind the row's earlier entries
__global__ __launch_bounds__(kThreads) void counted_append_kernel(const uint64_t *__restrict__ keys,
                                                                  const uint64_t *__restrict__ vals, int64_t n,
                                                                  const uint32_t *__restrict__ flag,
                                                                  const uint32_t *__restrict__ sum,
                                                                  const int64_t *__restrict__ pos,
                                                                  const MultiDesc *__restrict__ multi,
                                                                  const int64_t *__restrict__ off, int s,
                                                                  uint64_t *__restrict__ out, uint32_t *__restrict__ out_count,
                                                                  const int32_t *__restrict__ out_n) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const MultiDesc d = multi[vals[i] >> 32];
    const int64_t r = (int64_t)out_n[d.sketch] + (pos[i] - pos[off[d.part0]]);
    if (r < s) {
        out[(size_t)d.sketch * (size_t)s + r] = keys[i];
        out_count[(size_t)d.sketch * (size_t)s + r] = sum[i];
    }
}

// one thread per sketch with several chunks; pos == nullptr: nothing was gathered in this pass
__global__ __launch_bounds__(kThreads) void counted_finish_kernel(const MultiDesc *__restrict__ multi, int n_multi,
                                                                  int n_parts, int64_t total,
                                                                  const int64_t *__restrict__ off,
                                                                  const int64_t *__restrict__ pos,
                                                                  const uint64_t *__restrict__ multi_T, int s,
                                                                  SketchState st, int32_t *__restrict__ out_n) {
    const int m = blockIdx.x * kThreads + threadIdx.x;
    if (m >= n_multi) return;
    const MultiDesc d = multi[m];
    if (st.done[d.sketch]) return;
    int64_t added = 0;
    if (pos) {
        const int64_t b = off[d.part0], e = d.part0 + d.n_part < n_parts ? off[d.part0 + d.n_part] : total;
        added = pos[e] - pos[b];
    }
    const int n_new = (int)min((int64_t)s, (int64_t)out_n[d.sketch] + added);
    const uint64_t T = multi_T[m];
    out_n[d.sketch] = n_new;
    st.done[d.sketch] = (n_new >= s || T == ~0ull) ? 1 : 0;
    st.lo[d.sketch] = T + 1;
}

// one workgroup: the sketches that are not done
__global__ __launch_bounds__(kThreads) void counted_undone_kernel(const int32_t *__restrict__ done, int n,
                                                                  int64_t *__restrict__ out) {
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (int i = threadIdx.x; i < n; i += kThreads) mine += done[i] ? 0u : 1u;
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) *out = (int64_t)total;
}

// slots per chunk; 0: the default (hymet_sketch_counted_tune)
int &keep_setting() {
    static int k = 0;
    return k;
}
int keep_for(int s) { return keep_setting() > 0 ? keep_setting() : std::min(kMaxKeep, std::max(s, kDefaultKeep)); }

struct PassArgs {
    const uint32_t *d_2b, *d_mask;
    const CChunk *chunks;
    int64_t n_chunks;
    uint32_t seed;
    int s, keep;
    uint32_t min_copies;
    SketchState st;
    uint64_t *out;
    uint32_t *out_count;
    int32_t *out_n;
    uint64_t *part_h;
    uint32_t *part_c;
    PartMeta *part_meta;
    double alg_bytes;
};

template <int K>
int launch_chunks(hymet_ctx *ctx, const PassArgs &a) {
    const size_t lds = counted_lds(a.keep);
    if (lds > 64 * 1024)
        HY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&counted_chunk_kernel<K>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hymet::ProfScope _ps(ctx, "sketch_counted_chunk", a.alg_bytes);
    hipLaunchKernelGGL(counted_chunk_kernel<K>, dim3((unsigned)a.n_chunks), dim3(kThreads), lds, ctx->stream, a.d_2b, a.d_mask,
                       a.chunks, a.seed, a.s, a.keep, counted_cap(a.keep), a.min_copies, a.st, a.out, a.out_count, a.out_n, a.part_h, a.part_c,
                       a.part_meta);
    HY_CHECK_LAUNCH("counted_chunk_kernel");
    return HYMET_OK;
}

int launch_chunks_k(hymet_ctx *ctx, int k, const PassArgs &a) {
    switch (k) {
#define HY_K(KK) \
    case KK: return launch_chunks<KK>(ctx, a);
        HY_K(1) HY_K(2) HY_K(3) HY_K(4) HY_K(5) HY_K(6) HY_K(7) HY_K(8)
        HY_K(9) HY_K(10) HY_K(11) HY_K(12) HY_K(13) HY_K(14) HY_K(15) HY_K(16)
        HY_K(17) HY_K(18) HY_K(19) HY_K(20) HY_K(21) HY_K(22) HY_K(23) HY_K(24)
        HY_K(25) HY_K(26) HY_K(27) HY_K(28) HY_K(29) HY_K(30) HY_K(31) HY_K(32)
#undef HY_K
    }
    return hymet::fail(HYMET_E_ARG, "hymet_sketch_counted: k must be in 1..32");
}

}  // namespace

extern "C" {

int hymet_sketch_counted_max_size(void) { return kMaxKeep; }

int hymet_sketch_counted_tune(int keep) {
    HY_ARG(keep >= 0 && keep <= kMaxKeep, "hymet_sketch_counted_tune: keep in 0.." + std::to_string(kMaxKeep));
    keep_setting() = keep;
    return HYMET_OK;
}

int hymet_sketch_counted(hymet_ctx *ctx, const uint32_t *d_2b, const uint32_t *d_mask, int64_t n_bases, int k,
                         uint32_t seed, int32_t s, int32_t min_copies, int64_t n_chunks, const int32_t *h_chunk_sketch,
                         const int64_t *h_chunk_begin, const int64_t *h_chunk_end, int32_t n_sketches, uint64_t *d_out,
                         uint32_t *d_out_count, int32_t *d_out_n, int64_t *h_stats) {
    HY_ARG(ctx, "hymet_sketch_counted: null context");
    HY_ARG(k >= 1 && k <= 32, "hymet_sketch_counted: k must be in 1..32");
    HY_ARG(s >= 1 && s <= kMaxKeep, "hymet_sketch_counted: sketch size must be in 1.." + std::to_string(kMaxKeep));
    HY_ARG(min_copies >= 1, "hymet_sketch_counted: min_copies must be at least 1");
    HY_ARG(n_chunks >= 0 && n_sketches >= 0 && n_bases >= 0, "hymet_sketch_counted: negative count");
    HY_ARG(n_chunks < (1ll << 31) - 1, "hymet_sketch_counted: more than 2^31 - 2 chunks");
    if (h_stats) h_stats[0] = h_stats[1] = 0;
    if (n_sketches == 0) return HYMET_OK;
    HY_ARG(d_out && d_out_count && d_out_n, "hymet_sketch_counted: null output");
    HY_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    HY_HIP(hipMemsetAsync(d_out_n, 0, 4 * (size_t)n_sketches, st));  // sketches with no chunk: empty rows
    if (n_chunks == 0) return HYMET_OK;
    HY_ARG(d_2b && d_mask && h_chunk_sketch && h_chunk_begin && h_chunk_end, "hymet_sketch_counted: null argument");
    // the plan: everything is checked here, before any launch (hymet_sketch_batch's checks, and
    // the span of every sketch: the counts are 32 bits)
    const int64_t pos_end = n_bases - k + 1;  // one past the last k-mer start of the pool
    double bases = 0;
    {
        int64_t span = 0;
        for (int64_t c = 0; c < n_chunks; c++) {
            const int64_t b = h_chunk_begin[c], e = h_chunk_end[c];
            HY_ARG(h_chunk_sketch[c] >= 0 && h_chunk_sketch[c] < n_sketches,
                   "hymet_sketch_counted: chunk " + std::to_string(c) + ": sketch id out of range");
            HY_ARG(c == 0 || h_chunk_sketch[c] >= h_chunk_sketch[c - 1],
                   "hymet_sketch_counted: chunk " + std::to_string(c) + ": chunks are not sorted by sketch id");
            HY_ARG(b >= 0 && b <= e && e <= pos_end,
                   "hymet_sketch_counted: chunk " + std::to_string(c) + ": range outside [0, n_bases - k + 1)");
            if (c > 0 && h_chunk_sketch[c] != h_chunk_sketch[c - 1]) span = 0;
            span += e - b;
            HY_ARG(span < (1ll << 32), "hymet_sketch_counted: sketch " + std::to_string(h_chunk_sketch[c]) +
                                           " spans 2^32 positions or more (the counts are 32 bits)");
            bases += (double)(e - b);
        }
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
                   "hymet_sketch_counted: chunks " + std::to_string(last) + " and " + std::to_string(c) + " overlap");
            last = c;
        }
    }
    const int keep = keep_for(s);
    // a sketch with one chunk is finished by that chunk; the chunks of the others are parts
    std::vector<CChunk> cd((size_t)n_chunks);
    std::vector<MultiDesc> md;
    std::vector<int32_t> part_slot;
    std::vector<int32_t> done((size_t)n_sketches, 1);  // a sketch with no chunk is done: an empty row
    for (int64_t c = 0; c < n_chunks;) {
        int64_t e = c + 1;
        while (e < n_chunks && h_chunk_sketch[e] == h_chunk_sketch[c]) e++;
        const int32_t r = h_chunk_sketch[c];
        done[(size_t)r] = 0;
        if (e - c == 1) {
            cd[(size_t)c] = {h_chunk_begin[c], h_chunk_end[c], r, -1};
        } else {
            const int32_t slot = (int32_t)md.size();
            md.push_back({r, (int32_t)part_slot.size(), (int32_t)(e - c)});
            for (int64_t j = c; j < e; j++) {
                cd[(size_t)j] = {h_chunk_begin[j], h_chunk_end[j], r, (int32_t)part_slot.size()};
                part_slot.push_back(slot);
            }
        }
        c = e;
    }
    const int n_multi = (int)md.size(), n_parts = (int)part_slot.size();
    DevBuf d_chunks, d_multi, d_slot, d_lo, d_done, d_part_h, d_part_c, d_meta, d_T, d_take, d_off, d_undone;
    HY_HIP(d_chunks.alloc(sizeof(CChunk) * (size_t)n_chunks, st));
    HY_HIP(d_lo.alloc(8 * (size_t)n_sketches, st));
    HY_HIP(d_done.alloc(4 * (size_t)n_sketches, st));
    HY_HIP(d_undone.alloc(8, st));
    HY_HIP(hipMemcpyAsync(d_chunks.p, cd.data(), sizeof(CChunk) * (size_t)n_chunks, hipMemcpyHostToDevice, st));
    HY_HIP(hipMemsetAsync(d_lo.p, 0, 8 * (size_t)n_sketches, st));
    HY_HIP(hipMemcpyAsync(d_done.p, done.data(), 4 * (size_t)n_sketches, hipMemcpyHostToDevice, st));
    if (n_multi) {
        HY_HIP(d_multi.alloc(sizeof(MultiDesc) * (size_t)n_multi, st));
        HY_HIP(d_slot.alloc(4 * (size_t)n_parts, st));
        HY_HIP(d_part_h.alloc(8 * (size_t)n_parts * (size_t)keep, st));
        HY_HIP(d_part_c.alloc(4 * (size_t)n_parts * (size_t)keep, st));
        HY_HIP(d_meta.alloc(sizeof(PartMeta) * (size_t)n_parts, st));
        HY_HIP(d_T.alloc(8 * (size_t)n_multi, st));
        HY_HIP(d_take.alloc(4 * (size_t)n_parts, st));
        HY_HIP(d_off.alloc(8 * (size_t)(n_parts + 1), st));
        HY_HIP(hipMemcpyAsync(d_multi.p, md.data(), sizeof(MultiDesc) * (size_t)n_multi, hipMemcpyHostToDevice, st));
        HY_HIP(hipMemcpyAsync(d_slot.p, part_slot.data(), 4 * (size_t)n_parts, hipMemcpyHostToDevice, st));
    }
    const SketchState state{d_lo.as<uint64_t>(), d_done.as<int32_t>()};
    const PassArgs pa{d_2b, d_mask, d_chunks.as<CChunk>(), n_chunks, seed, (int)s, keep, (uint32_t)min_copies, state,
                      d_out, d_out_count, d_out_n, d_part_h.as<uint64_t>(), d_part_c.as<uint32_t>(), d_meta.as<PartMeta>(),
                      0.375 * bases + (double)kSlotBytes * (double)keep * (double)n_chunks};
    const MultiDesc *dm = d_multi.as<MultiDesc>();
    const int hash_bits = k <= 16 ? 32 : 64;
    int64_t passes = 0, merged = 0, undone = 0;
    do {
        int rc = launch_chunks_k(ctx, k, pa);
        if (rc) return rc;
        if (n_multi) {
            hymet::ProfScope _ps(ctx, "sketch_counted_merge");
            hipLaunchKernelGGL(counted_threshold_kernel, dim3((unsigned)n_multi), dim3(kThreads), 0, st, dm, keep, state,
                               d_part_h.as<uint64_t>(), d_meta.as<PartMeta>(), d_T.as<uint64_t>(), d_take.as<uint32_t>());
            HY_CHECK_LAUNCH("counted_threshold_kernel");
            int64_t total = 0;
            rc = hymet::mm::exclusive_scan_u32_i64(ctx, d_take.as<uint32_t>(), d_off.as<int64_t>(), n_parts, &total);
            if (rc) return rc;
            DevBuf keys, keys_alt, vals, vals_alt, flag, sum, pos, scan_part;
            if (total > 0) {
                merged += total;
                HY_HIP(keys.alloc(8 * (size_t)total, st));
                HY_HIP(keys_alt.alloc(8 * (size_t)total, st));
                HY_HIP(vals.alloc(8 * (size_t)total, st));
                HY_HIP(vals_alt.alloc(8 * (size_t)total, st));
                HY_HIP(flag.alloc(4 * (size_t)(total + 1), st));
                HY_HIP(sum.alloc(4 * (size_t)total, st));
                HY_HIP(pos.alloc(8 * (size_t)(total + 1), st));
                uint64_t *pk = keys.as<uint64_t>(), *pka = keys_alt.as<uint64_t>();
                uint64_t *pv = vals.as<uint64_t>(), *pva = vals_alt.as<uint64_t>();
                hipLaunchKernelGGL(counted_gather_kernel, dim3((unsigned)n_parts), dim3(kThreads), 0, st, keep,
                                   d_slot.as<int32_t>(), d_part_h.as<uint64_t>(), d_part_c.as<uint32_t>(),
                                   d_take.as<uint32_t>(), d_off.as<int64_t>(), pk, pv);
                HY_CHECK_LAUNCH("counted_gather_kernel");
                // by hash, then stably by slot: the pairs of a sketch end up together, hashes ascending
                rc = hymet::mm::radix_sort_pairs(ctx, pk, pka, pv, pva, total, 0, hash_bits);
                if (rc) return rc;
                if (n_multi > 1) {
                    rc = hymet::mm::radix_sort_pairs(ctx, pv, pva, pk, pka, total, 32, 32 + hymet::mm::bits_for(n_multi - 1));
                    if (rc) return rc;
                }
                const unsigned nb = (unsigned)hymet::cdiv(total + 1, kThreads);
                hipLaunchKernelGGL(counted_flag_kernel, dim3(nb), dim3(kThreads), 0, st, pk, pv, total, (uint32_t)min_copies,
                                   flag.as<uint32_t>(), sum.as<uint32_t>());
                HY_CHECK_LAUNCH("counted_flag_kernel");
                rc = hymet::mm::scan_u32_i64(ctx, flag.as<uint32_t>(), pos.as<int64_t>(), total + 1, scan_part);
                if (rc) return rc;
                hipLaunchKernelGGL(counted_append_kernel, dim3(nb), dim3(kThreads), 0, st, pk, pv, total, flag.as<uint32_t>(),
                                   sum.as<uint32_t>(), pos.as<int64_t>(), dm, d_off.as<int64_t>(), (int)s, d_out, d_out_count,
                                   d_out_n);
                HY_CHECK_LAUNCH("counted_append_kernel");
            }
            hipLaunchKernelGGL(counted_finish_kernel, dim3((unsigned)hymet::cdiv(n_multi, kThreads)), dim3(kThreads), 0, st, dm,
                               n_multi, n_parts, total, d_off.as<int64_t>(), total > 0 ? pos.as<int64_t>() : nullptr,
                               d_T.as<uint64_t>(), (int)s, state, d_out_n);
            HY_CHECK_LAUNCH("counted_finish_kernel");
        }
        hipLaunchKernelGGL(counted_undone_kernel, dim3(1), dim3(kThreads), 0, st, d_done.as<int32_t>(), (int)n_sketches,
                           d_undone.as<int64_t>());
        HY_CHECK_LAUNCH("counted_undone_kernel");
        HY_HIP(hipMemcpyAsync(&undone, d_undone.p, 8, hipMemcpyDeviceToHost, st));
        HY_HIP(hipStreamSynchronize(st));
        passes++;
    } while (undone > 0);
    if (h_stats) {
        h_stats[0] = passes;
        h_stats[1] = merged;
    }
    return HYMET_OK;
}

}  // extern "C"

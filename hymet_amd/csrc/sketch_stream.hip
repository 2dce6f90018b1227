// Mash `sketch -r -m M` of a read set that does not fit in one batch: the file is read once per
// pass, in batches, and a small state stays in HBM between them (DESIGN.md §3 "Sketch: read
// sets, streamed").  The result is sketch_counted.hip's -- the s smallest canonical k-mer hashes
// seen at least M times in the whole read set, with their multiplicities -- and like it exact,
// with no threshold supplied or guessed, and independent of how the input was cut.
//
// The state of one read set (hymet_sketch_stream): the row written so far (row_n <= s entries),
// a hash window [lo, hi] and `live`, the ascending list of the DISTINCT (hash, count) pairs of
// every hash in the window seen so far in this pass.  lo, hi and live_n live in device memory
// (StreamState).  A pass starts with hi = all ones and live empty; per slice of a batch:
//   stream_emit<K>   rolls over the slice (KmerRoll<K>, the tiles and warm-up of
//                    counted_chunk_kernel) and appends every hash in [lo, hi] to a candidate
//                    buffer with room for every k-mer start of the slice: one wave-aggregated
//                    atomic on a cursor per wave and step.  The order of the candidates is the
//                    schedule's; the sort that follows removes it.
//   radix sort       (sort.hpp) of the candidates, over the bits up to hi's highest set bit
//   stream_heads / scan / stream_runs: the slice's distinct hashes and where each one's run of
//                    copies starts (its count = the next start - its own)
//   merge path       stream_partition cuts the merged order of live (A) and the slice (B) into
//                    tiles of 2,048 by binary search on the diagonals (ties: A first), then
//                    stream_merge<false> flags the B entries that have no equal in A, a scan
//                    ranks them, and stream_merge<true> writes every A entry (its count plus its
//                    equal's, saturating at 2^32 - 1) and every flagged B entry to its place:
//                    index in A + flagged B entries before it.  The searches run on the tile's
//                    hashes in LDS; live is never sorted again.
//   stream_tighten   need = s - row_n; when the merged list holds need entries with count >= M,
//                    hi falls to the need-th of them and everything above it is dropped (the list
//                    ascends: live_n shrinks).  Then the forced cut: a list longer than max_live
//                    is cut to its max_live / 2 smallest, hi falls to the last of them, and the
//                    pass is marked cut.
// hi only falls, so every entry kept was inside the window at every one of its occurrences: its
// count is complete.  At the end of a pass the entries with count >= M go to the row by rank; the
// read set is finished when the row is full or the pass was never cut, else lo = hi + 1 and the
// file is read again.
//
// A batch is cut into slices of slice_bases k-mer starts, shorter ones while the window is open
// (kFirstSlice).  One host synchronisation per slice: the candidate count (the sort's launch needs it), read
// together with hi and live_n in one 64-byte copy.  A slice that emitted nothing ends there.
// Integer work only; the row is written by rank, no atomics on it.
#include "sort.hpp"
#include "mash_hash.hpp"

namespace {

using namespace hymet::mash;
using hymet::mm::DevBuf;

constexpr int kThreads = 256;
constexpr int kTile = 64;           // k-mer starts per thread (the screen's tile)
constexpr int kMergeTile = 2048;    // merged entries per workgroup of the merge: 16 KiB of LDS
// While the window is still open (hi = all ones) every hash of a slice is a candidate and is
// sorted over all its bits, so a pass starts with slices of 2^20 k-mer starts, doubled until hi
// has fallen or slice_bases is reached.  The result does not depend on it.
constexpr int64_t kFirstSlice = 1 << 20;

struct StreamState {
    uint64_t lo, hi;                // the window; hashes below lo are dealt with
    unsigned long long cand_n;      // the emit cursor; zero between slices
    int64_t live_n;
    int64_t slice_n;                // distinct hashes of the slice being merged
    int64_t max_live;               // the largest live_n a merge produced (before tightening)
    int32_t row_n, cut, finished, pad;
};

template <int K>
__global__ __launch_bounds__(kThreads) void stream_emit_kernel(const uint32_t *__restrict__ w2b,
                                                               const uint32_t *__restrict__ wm, int64_t begin, int64_t end,
                                                               uint32_t seed, StreamState *st, uint64_t *__restrict__ cand) {
    const uint64_t lo = st->lo, hi = st->hi;
    const int64_t p0 = begin + ((int64_t)blockIdx.x * kThreads + threadIdx.x) * kTile;  // first k-mer start
    const int64_t p1 = min(p0 + kTile, end);                                            // one past the last
    const int lane = threadIdx.x & 63;
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
    if (p0 < end)
        for (int j = 0; j < K - 1; j++) step();
#pragma unroll 1
    for (int j = 0; j < kTile; j++) {
        bool ok = p0 + j < p1;  // this start belongs to the thread's tile
        uint64_t h = 0;
        if (ok) {
            step();
            ok = run >= K;  // no invalid base inside the k-mer
            if (ok) h = roll.hash(seed);
        }
        const bool acc = ok && h >= lo && h <= hi;
        const uint64_t m = __ballot(acc);
        if (m == 0) continue;  // wave-uniform
        const int leader = __ffsll((unsigned long long)m) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(&st->cand_n, (unsigned long long)__popcll(m));
        base = __shfl(base, leader, 64);
        if (acc) cand[base + (unsigned long long)__popcll(m & ((1ull << lane) - 1))] = h;
    }
}

// flag has n + 1 entries, the last one 0, so that the scan ends with the number of distinct hashes
__global__ __launch_bounds__(kThreads) void stream_heads_kernel(const uint64_t *__restrict__ keys, int64_t n,
                                                                uint32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i > n) return;
    flag[i] = (i < n && (i == 0 || keys[i] != keys[i - 1])) ? 1u : 0u;
}

// the first of every run of equal hashes writes the hash and the run's start; start[slice_n] = n
__global__ __launch_bounds__(kThreads) void stream_runs_kernel(const uint64_t *__restrict__ keys, int64_t n,
                                                               const uint32_t *__restrict__ flag,
                                                               const int64_t *__restrict__ pos, uint64_t *__restrict__ sh,
                                                               int64_t *__restrict__ sstart, StreamState *st) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        sstart[pos[n]] = n;
        st->slice_n = pos[n];
    } else if (flag[i]) {
        sh[pos[i]] = keys[i];
        sstart[pos[i]] = i;
    }
}

// split[t]: how many entries of A lie before diagonal t * kMergeTile of the merged order (an A
// entry goes before an equal B entry); t in 0..n_tiles
__global__ __launch_bounds__(kThreads) void stream_partition_kernel(const uint64_t *__restrict__ A, int64_t nA,
                                                                    const uint64_t *__restrict__ B, const StreamState *st,
                                                                    int64_t n_tiles, int64_t *__restrict__ split) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t > n_tiles) return;
    const int64_t nB = st->slice_n;
    const int64_t d = min(t * kMergeTile, nA + nB);
    int64_t lo = max((int64_t)0, d - nB), hi = min(d, nA);
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (A[mid] <= B[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    split[t] = lo;
}

__device__ __forceinline__ uint32_t sat32(uint64_t v) { return v > 0xffffffffull ? 0xffffffffu : (uint32_t)v; }

// One tile of the merged order: A[i0, i1) and B[j0, j1), the hashes of both in LDS.  By the
// partition A[i0 - 1] <= B[j0], B[j0 - 1] < A[i0], A[i1 - 1] <= B[j1] and B[j1 - 1] < A[i1], so
// an entry's rank in the other list is its rank in the other list's part of the tile.
//   WRITE = false: f[j] = 1 for every B entry with no equal in A
//   WRITE = true : pf = the exclusive scan of f.  A[i] goes to i + pf[j], j = the B entries below
//                  it, with B[j]'s count added when B[j] is its equal; a flagged B[j] goes to
//                  (the A entries <= it) + pf[j].  qflag[p] = 1 where the count written at p
//                  reaches min_copies (zeroed by the caller, n_out and beyond stay 0).
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void stream_merge_kernel(const uint64_t *__restrict__ Ah, const uint32_t *__restrict__ Ac,
                                                                int64_t nA, const uint64_t *__restrict__ Bh,
                                                                const int64_t *__restrict__ Bstart, StreamState *st,
                                                                const int64_t *__restrict__ split, uint32_t *__restrict__ f,
                                                                const int64_t *__restrict__ pf, uint64_t *__restrict__ oh,
                                                                uint32_t *__restrict__ oc, uint32_t *__restrict__ qflag,
                                                                uint32_t min_copies) {
    __shared__ uint64_t sm[kMergeTile];
    const int64_t nB = st->slice_n;
    const int64_t d0 = min((int64_t)blockIdx.x * kMergeTile, nA + nB), d1 = min(d0 + kMergeTile, nA + nB);
    const int64_t i0 = split[blockIdx.x], i1 = split[blockIdx.x + 1];
    const int64_t j0 = d0 - i0, j1 = d1 - i1;
    const int na = (int)(i1 - i0), nb = (int)(j1 - j0);
    const uint64_t *sa = sm, *sb = sm + na;
    for (int e = threadIdx.x; e < na + nb; e += kThreads) sm[e] = e < na ? Ah[i0 + e] : Bh[j0 + (e - na)];
    __syncthreads();
    if (WRITE && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t n_out = nA + pf[nB];
        st->live_n = n_out;
        if (n_out > st->max_live) st->max_live = n_out;
    }
    for (int e = threadIdx.x; e < na + nb; e += kThreads) {
        if (e < na) {
            if (!WRITE) continue;
            const uint64_t a = sa[e];
            int l = 0, r = nb;  // the B entries of the tile below a
            while (l < r) {
                const int mid = (l + r) >> 1;
                if (sb[mid] < a) l = mid + 1;
                else r = mid;
            }
            const int64_t j = j0 + l;
            const bool both = l < nb ? sb[l] == a : (j < nB && Bh[j] == a);  // its equal may open the next tile
            uint64_t c = Ac[i0 + e];
            if (both) c += (uint64_t)(Bstart[j + 1] - Bstart[j]);
            const int64_t p = i0 + e + pf[j];
            oh[p] = a;
            oc[p] = sat32(c);
            if (sat32(c) >= min_copies) qflag[p] = 1u;
        } else {
            const int jl = e - na;
            const uint64_t b = sb[jl];
            int l = 0, r = na;  // the A entries of the tile at or below b
            while (l < r) {
                const int mid = (l + r) >> 1;
                if (sa[mid] <= b) l = mid + 1;
                else r = mid;
            }
            const bool dup = l > 0 ? sa[l - 1] == b : (i0 > 0 && Ah[i0 - 1] == b);  // its equal may close the last tile
            const int64_t j = j0 + jl;
            if (!WRITE) {
                f[j] = dup ? 0u : 1u;
            } else if (!dup) {
                const uint32_t c = sat32((uint64_t)(Bstart[j + 1] - Bstart[j]));
                const int64_t p = i0 + l + pf[j];
                oh[p] = b;
                oc[p] = c;
                if (c >= min_copies) qflag[p] = 1u;
            }
        }
    }
}

// qpos = the exclusive scan of qflag over nU + 1 entries (qflag[nU] = 0): qpos[nU] entries qualify.
// The need-th qualifier, when there is one, closes the window behind itself; thread 0 speaks for
// the list when there is none.  Whoever decides also applies the forced cut and clears the
// emit cursor for the next slice: one thread writes, nobody reads what it writes.
__global__ __launch_bounds__(kThreads) void stream_tighten_kernel(const uint64_t *__restrict__ oh,
                                                                  const uint32_t *__restrict__ qflag,
                                                                  const int64_t *__restrict__ qpos, int64_t nU, int s,
                                                                  int64_t max_live, StreamState *st) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= nU) return;
    const int64_t need = (int64_t)s - st->row_n;
    const bool found = qflag[i] && qpos[i] == need - 1;
    if (!found && !(i == 0 && qpos[nU] < need)) return;
    int64_t n = found ? i + 1 : st->live_n;
    bool cut = false;
    if (n > max_live) {
        n = max_live / 2;
        cut = true;
    }
    if (found || cut) st->hi = oh[n - 1];
    if (cut) st->cut = 1;
    st->live_n = n;
    st->cand_n = 0;
}

// end of a pass: flag has n + 1 entries, the last one 0
__global__ __launch_bounds__(kThreads) void stream_qual_kernel(const uint32_t *__restrict__ c, int64_t n, uint32_t min_copies,
                                                               uint32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i > n) return;
    flag[i] = (i < n && c[i] >= min_copies) ? 1u : 0u;
}

// a qualifier's rank places it behind the row's earlier entries
__global__ __launch_bounds__(kThreads) void stream_append_kernel(const uint64_t *__restrict__ h, const uint32_t *__restrict__ c,
                                                                 int64_t n, const uint32_t *__restrict__ flag,
                                                                 const int64_t *__restrict__ pos, int s,
                                                                 const StreamState *st, uint64_t *__restrict__ row,
                                                                 uint32_t *__restrict__ rowc) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int64_t r = (int64_t)st->row_n + pos[i];
    if (r < s) {
        row[r] = h[i];
        rowc[r] = c[i];
    }
}

// one thread; total: the pass's qualifiers (nullptr: live was empty)
__global__ void stream_finish_kernel(const int64_t *total, int s, StreamState *st) {
    const int64_t q = total ? *total : 0;
    const int32_t n_new = (int32_t)min((int64_t)s, (int64_t)st->row_n + q);
    st->row_n = n_new;
    st->finished = (n_new >= s || !st->cut || st->hi == ~0ull) ? 1 : 0;
    st->lo = st->hi + 1;
    st->hi = ~0ull;
    st->live_n = 0;
    st->cut = 0;
}

struct EmitArgs {
    const uint32_t *d_2b, *d_mask;
    int64_t begin, end;
    uint32_t seed;
    StreamState *st;
    uint64_t *cand;
};

template <int K>
int launch_emit(hymet_ctx *ctx, const EmitArgs &a) {
    hymet::ProfScope _ps(ctx, "sketch_stream_emit", 0.375 * (double)(a.end - a.begin));
    const unsigned nb = (unsigned)hymet::cdiv(a.end - a.begin, (int64_t)kThreads * kTile);
    hipLaunchKernelGGL(stream_emit_kernel<K>, dim3(nb), dim3(kThreads), 0, ctx->stream, a.d_2b, a.d_mask, a.begin, a.end, a.seed,
                       a.st, a.cand);
    HY_CHECK_LAUNCH("stream_emit_kernel");
    return HYMET_OK;
}

int launch_emit_k(hymet_ctx *ctx, int k, const EmitArgs &a) {
    switch (k) {
#define HY_K(KK) \
    case KK: return launch_emit<KK>(ctx, a);
        HY_K(1) HY_K(2) HY_K(3) HY_K(4) HY_K(5) HY_K(6) HY_K(7) HY_K(8)
        HY_K(9) HY_K(10) HY_K(11) HY_K(12) HY_K(13) HY_K(14) HY_K(15) HY_K(16)
        HY_K(17) HY_K(18) HY_K(19) HY_K(20) HY_K(21) HY_K(22) HY_K(23) HY_K(24)
        HY_K(25) HY_K(26) HY_K(27) HY_K(28) HY_K(29) HY_K(30) HY_K(31) HY_K(32)
#undef HY_K
    }
    return hymet::fail(HYMET_E_ARG, "hymet_sketch_stream_add: k must be in 1..32");
}

inline unsigned blocks_for(int64_t n) { return (unsigned)hymet::cdiv(n, kThreads); }

}  // namespace

// opaque handle (include/hymet_gpu.h)
struct hymet_sketch_stream {
    hymet_ctx *ctx = nullptr;
    int k = 0, s = 0;
    uint32_t seed = 0, min_copies = 1;
    int64_t max_live = 0;
    DevBuf state, live_h, live_c, row_h, row_c;
    bool finished = false;
    bool failed = false;  // a call failed half-way: the device state is unknown, nothing more is taken
    bool tight = false;   // this pass's window has fallen below all ones (as of the last readback)
    int64_t open_slice = kFirstSlice;  // the slice length while it has not
    int32_t row_n = 0;
    int64_t passes = 0, slices = 0, emitted = 0, max_live_seen = 0;
};

namespace {

int read_state(hymet_sketch_stream *S, StreamState *h) {
    HY_HIP(hipMemcpyAsync(h, S->state.p, sizeof(StreamState), hipMemcpyDeviceToHost, S->ctx->stream));
    HY_HIP(hipStreamSynchronize(S->ctx->stream));
    return HYMET_OK;
}

// sort + reduce + merge + tighten of one slice's n candidates; nA = live_n, hi as the emit read it
int merge_slice(hymet_sketch_stream *S, DevBuf &cand, int64_t n, int64_t nA, uint64_t hi) {
    hymet_ctx *ctx = S->ctx;
    hipStream_t st = ctx->stream;
    StreamState *ds = S->state.as<StreamState>();
    hymet::ProfScope _ps(ctx, "sketch_stream_merge");
    // the slice's distinct hashes (sh) and the starts of their runs of copies (sstart)
    DevBuf keys_alt, vals, vals_alt, flag, pos, scan_part, sh, sstart;
    HY_HIP(keys_alt.alloc(8 * (size_t)n, st));
    HY_HIP(vals.alloc((size_t)n, st));      // the pair sort's values: unused bytes
    HY_HIP(vals_alt.alloc((size_t)n, st));
    uint64_t *pk = cand.as<uint64_t>(), *pka = keys_alt.as<uint64_t>();
    uint8_t *pv = vals.as<uint8_t>(), *pva = vals_alt.as<uint8_t>();
    const int hash_bits = S->k <= 16 ? 32 : 64;
    const int hi_bits = hi == 0 ? 1 : 64 - __builtin_clzll((unsigned long long)hi);
    int rc = hymet::mm::radix_sort_pairs(ctx, pk, pka, pv, pva, n, 0, std::min(hash_bits, hi_bits));
    if (rc) return rc;
    HY_HIP(flag.alloc(4 * (size_t)(n + 1), st));
    HY_HIP(pos.alloc(8 * (size_t)(n + 1), st));
    HY_HIP(sh.alloc(8 * (size_t)n, st));
    HY_HIP(sstart.alloc(8 * (size_t)(n + 1), st));
    hipLaunchKernelGGL(stream_heads_kernel, dim3(blocks_for(n + 1)), dim3(kThreads), 0, st, pk, n, flag.as<uint32_t>());
    HY_CHECK_LAUNCH("stream_heads_kernel");
    rc = hymet::mm::scan_u32_i64(ctx, flag.as<uint32_t>(), pos.as<int64_t>(), n + 1, scan_part);
    if (rc) return rc;
    hipLaunchKernelGGL(stream_runs_kernel, dim3(blocks_for(n + 1)), dim3(kThreads), 0, st, pk, n, flag.as<uint32_t>(),
                       pos.as<int64_t>(), sh.as<uint64_t>(), sstart.as<int64_t>(), ds);
    HY_CHECK_LAUNCH("stream_runs_kernel");
    // merge path: live (nA entries) and the slice (slice_n <= n entries) into a new list
    const int64_t nU = nA + n, n_tiles = hymet::cdiv(nU, kMergeTile);
    DevBuf split, f, pf, scan_part2, oh, oc, qflag, qpos, scan_part3;
    HY_HIP(split.alloc(8 * (size_t)(n_tiles + 1), st));
    HY_HIP(f.alloc(4 * (size_t)(n + 1), st));
    HY_HIP(pf.alloc(8 * (size_t)(n + 1), st));
    HY_HIP(oh.alloc(8 * (size_t)nU, st));
    HY_HIP(oc.alloc(4 * (size_t)nU, st));
    HY_HIP(qflag.alloc(4 * (size_t)(nU + 1), st));
    HY_HIP(qpos.alloc(8 * (size_t)(nU + 1), st));
    HY_HIP(hipMemsetAsync(f.p, 0, 4 * (size_t)(n + 1), st));
    HY_HIP(hipMemsetAsync(qflag.p, 0, 4 * (size_t)(nU + 1), st));
    const uint64_t *Ah = S->live_h.as<uint64_t>();
    const uint32_t *Ac = S->live_c.as<uint32_t>();
    hipLaunchKernelGGL(stream_partition_kernel, dim3(blocks_for(n_tiles + 1)), dim3(kThreads), 0, st, Ah, nA, sh.as<uint64_t>(),
                       ds, n_tiles, split.as<int64_t>());
    HY_CHECK_LAUNCH("stream_partition_kernel");
    hipLaunchKernelGGL(stream_merge_kernel<false>, dim3((unsigned)n_tiles), dim3(kThreads), 0, st, Ah, Ac, nA, sh.as<uint64_t>(),
                       sstart.as<int64_t>(), ds, split.as<int64_t>(), f.as<uint32_t>(), pf.as<int64_t>(), oh.as<uint64_t>(),
                       oc.as<uint32_t>(), qflag.as<uint32_t>(), S->min_copies);
    HY_CHECK_LAUNCH("stream_merge_kernel<false>");
    rc = hymet::mm::scan_u32_i64(ctx, f.as<uint32_t>(), pf.as<int64_t>(), n + 1, scan_part2);
    if (rc) return rc;
    hipLaunchKernelGGL(stream_merge_kernel<true>, dim3((unsigned)n_tiles), dim3(kThreads), 0, st, Ah, Ac, nA, sh.as<uint64_t>(),
                       sstart.as<int64_t>(), ds, split.as<int64_t>(), f.as<uint32_t>(), pf.as<int64_t>(), oh.as<uint64_t>(),
                       oc.as<uint32_t>(), qflag.as<uint32_t>(), S->min_copies);
    HY_CHECK_LAUNCH("stream_merge_kernel<true>");
    rc = hymet::mm::scan_u32_i64(ctx, qflag.as<uint32_t>(), qpos.as<int64_t>(), nU + 1, scan_part3);
    if (rc) return rc;
    hipLaunchKernelGGL(stream_tighten_kernel, dim3(blocks_for(nU)), dim3(kThreads), 0, st, oh.as<uint64_t>(), qflag.as<uint32_t>(),
                       qpos.as<int64_t>(), nU, S->s, S->max_live, ds);
    HY_CHECK_LAUNCH("stream_tighten_kernel");
    S->live_h.swap(oh);  // the old list goes back to the scratch cache behind the kernels that read it
    S->live_c.swap(oc);
    return HYMET_OK;
}

}  // namespace

extern "C" {

int hymet_sketch_stream_create(hymet_ctx *ctx, int k, uint32_t seed, int32_t s, int32_t min_copies, int64_t max_live,
                               hymet_sketch_stream **out) {
    HY_ARG(ctx && out, "hymet_sketch_stream_create: null argument");
    HY_ARG(k >= 1 && k <= 32, "hymet_sketch_stream_create: k must be in 1..32");
    HY_ARG(s >= 1 && s <= hymet_sketch_counted_max_size(),
           "hymet_sketch_stream_create: sketch size must be in 1.." + std::to_string(hymet_sketch_counted_max_size()));
    HY_ARG(min_copies >= 1, "hymet_sketch_stream_create: min_copies must be at least 1");
    HY_ARG(max_live >= 2, "hymet_sketch_stream_create: max_live must be at least 2");
    HY_HIP(hipSetDevice(ctx->device));
    hymet_sketch_stream *S = new hymet_sketch_stream();
    S->ctx = ctx;
    S->k = k;
    S->s = s;
    S->seed = seed;
    S->min_copies = (uint32_t)min_copies;
    S->max_live = max_live;
    hipStream_t st = ctx->stream;
    StreamState init{};
    init.hi = ~0ull;
    hipError_t e = S->state.alloc(sizeof(StreamState), st);
    if (e == hipSuccess) e = S->row_h.alloc(8 * (size_t)s, st);
    if (e == hipSuccess) e = S->row_c.alloc(4 * (size_t)s, st);
    if (e == hipSuccess) e = hipMemcpyAsync(S->state.p, &init, sizeof(init), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        delete S;
        return hymet::hip_fail(e, "hymet_sketch_stream_create");
    }
    *out = S;
    return HYMET_OK;
}

int hymet_sketch_stream_add(hymet_sketch_stream *S, const uint32_t *d_2b, const uint32_t *d_mask, int64_t n_bases,
                            int64_t slice_bases) {
    HY_ARG(S, "hymet_sketch_stream_add: null handle");
    HY_ARG(!S->finished, "hymet_sketch_stream_add: the read set is finished");
    HY_ARG(!S->failed, "hymet_sketch_stream_add: an earlier call on this handle failed");
    HY_ARG(n_bases >= 0, "hymet_sketch_stream_add: negative count");
    HY_ARG(slice_bases >= 1, "hymet_sketch_stream_add: slice_bases must be at least 1");
    const int64_t pos_end = n_bases - S->k + 1;  // one past the last k-mer start of the batch
    if (pos_end <= 0) return HYMET_OK;
    HY_ARG(d_2b && d_mask, "hymet_sketch_stream_add: null argument");
    hymet_ctx *ctx = S->ctx;
    HY_HIP(hipSetDevice(ctx->device));
    S->failed = true;  // until every slice is through
    for (int64_t b = 0; b < pos_end;) {
        const int64_t len = S->tight ? slice_bases : std::min(slice_bases, S->open_slice);
        const int64_t e = len < pos_end - b ? b + len : pos_end;
        DevBuf cand;  // room for every k-mer start of the slice: the emit cannot overflow it
        HY_HIP(cand.alloc(8 * (size_t)(e - b), ctx->stream));
        int rc = launch_emit_k(ctx, S->k, EmitArgs{d_2b, d_mask, b, e, S->seed, S->state.as<StreamState>(), cand.as<uint64_t>()});
        if (rc) return rc;
        StreamState h;
        rc = read_state(S, &h);
        if (rc) return rc;
        S->slices++;
        S->emitted += (int64_t)h.cand_n;
        if (h.hi != ~0ull) S->tight = true;
        else if (S->open_slice < (1ll << 40)) S->open_slice *= 2;
        if (h.cand_n > 0) {
            rc = merge_slice(S, cand, (int64_t)h.cand_n, h.live_n, h.hi);
            if (rc) return rc;
        }
        b = e;
    }
    S->failed = false;
    return HYMET_OK;
}

int hymet_sketch_stream_end_pass(hymet_sketch_stream *S, int32_t *need_more) {
    HY_ARG(S && need_more, "hymet_sketch_stream_end_pass: null argument");
    *need_more = 0;
    if (S->finished) return HYMET_OK;
    HY_ARG(!S->failed, "hymet_sketch_stream_end_pass: an earlier call on this handle failed");
    hymet_ctx *ctx = S->ctx;
    HY_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    StreamState *ds = S->state.as<StreamState>();
    StreamState h;
    int rc = read_state(S, &h);
    if (rc) return rc;
    const int64_t n = h.live_n;
    DevBuf flag, pos, scan_part;
    if (n > 0) {
        HY_HIP(flag.alloc(4 * (size_t)(n + 1), st));
        HY_HIP(pos.alloc(8 * (size_t)(n + 1), st));
        hipLaunchKernelGGL(stream_qual_kernel, dim3(blocks_for(n + 1)), dim3(kThreads), 0, st, S->live_c.as<uint32_t>(), n,
                           S->min_copies, flag.as<uint32_t>());
        HY_CHECK_LAUNCH("stream_qual_kernel");
        rc = hymet::mm::scan_u32_i64(ctx, flag.as<uint32_t>(), pos.as<int64_t>(), n + 1, scan_part);
        if (rc) return rc;
        hipLaunchKernelGGL(stream_append_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, st, S->live_h.as<uint64_t>(),
                           S->live_c.as<uint32_t>(), n, flag.as<uint32_t>(), pos.as<int64_t>(), S->s, ds, S->row_h.as<uint64_t>(),
                           S->row_c.as<uint32_t>());
        HY_CHECK_LAUNCH("stream_append_kernel");
    }
    hipLaunchKernelGGL(stream_finish_kernel, dim3(1), dim3(1), 0, st, n > 0 ? pos.as<int64_t>() + n : nullptr, S->s, ds);
    HY_CHECK_LAUNCH("stream_finish_kernel");
    rc = read_state(S, &h);
    if (rc) return rc;
    S->passes++;
    S->tight = false;
    S->open_slice = kFirstSlice;
    S->row_n = h.row_n;
    S->max_live_seen = h.max_live;
    S->finished = h.finished != 0;
    if (S->finished) {  // the list is of no further use
        S->live_h.release();
        S->live_c.release();
    }
    *need_more = S->finished ? 0 : 1;
    return HYMET_OK;
}

int hymet_sketch_stream_result(hymet_sketch_stream *S, uint64_t *d_out, uint32_t *d_out_count, int32_t *n, int64_t *h_stats) {
    HY_ARG(S && n, "hymet_sketch_stream_result: null argument");
    HY_ARG(S->finished, "hymet_sketch_stream_result: the read set is not finished (end_pass asked for another pass)");
    HY_ARG(S->row_n == 0 || (d_out && d_out_count), "hymet_sketch_stream_result: null output");
    hymet_ctx *ctx = S->ctx;
    HY_HIP(hipSetDevice(ctx->device));
    if (S->row_n > 0) {
        HY_HIP(hipMemcpyAsync(d_out, S->row_h.p, 8 * (size_t)S->row_n, hipMemcpyDeviceToDevice, ctx->stream));
        HY_HIP(hipMemcpyAsync(d_out_count, S->row_c.p, 4 * (size_t)S->row_n, hipMemcpyDeviceToDevice, ctx->stream));
        HY_HIP(hipStreamSynchronize(ctx->stream));
    }
    *n = S->row_n;
    if (h_stats) {
        h_stats[0] = S->passes;
        h_stats[1] = S->slices;
        h_stats[2] = S->emitted;
        h_stats[3] = S->max_live_seen;
    }
    return HYMET_OK;
}

int hymet_sketch_stream_destroy(hymet_sketch_stream *S) {
    if (S) {
        (void)hipSetDevice(S->ctx->device);
        delete S;
    }
    return HYMET_OK;
}

}  // extern "C"

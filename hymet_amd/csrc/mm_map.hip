// Mapping of query contigs against one minimizer-index part with minimap2's asm10 settings
// (replaces `minimap2 -x asm10 reference.mmi input/ *.fna`, scripts/minimap2.sh:23;
// SURVEY.md §3.4, §8a rows A2-A4).  Stage by stage (map.c mm_map_frag):
//   1 sketch every query (mm_sketch_kernel, rid 0)
//   2 mm_seed_mz_flt: per-query over-represented minimizers (an LDS bucket screen per query;
//     a (query, x) radix sort + run count only for the queries it cannot clear)
//   3 seeds: CSR lookup of every minimizer (two adjacent loads), then one thread per query
//     replays mm_seed_select / mm_collect_matches (high-occurrence streaks, rep_len,
//     mini_pos) -- sequential by nature but O(minimizers) and parallel over queries
//   4 anchors: exclusive scan of seed occurrence counts, one thread per seed writes them
//   5 sort anchors by (query, strand, target, tpos, qpos): the grouped per-query sort of
//     mm_asort.hip (block sorts in LDS; the library's LSD radix sort only for groups of
//     more than 16384 anchors); a layout without an anchor word takes the two-key fallback
//   6 chain_set (mm_chainset.hip): groups (query, strand, target) -> chain_groups_kernel (one
//     wave per group) -> backtrack_groups_kernel -> chains ordered by first anchor (compact_a)
//   7 long-join re-chain with bw_long for the queries that need it: their chained anchors,
//     compacted out of the sorted first-pass set by the backtrack's marks
//   8 one thread per query: mm_gen_regs, mm_set_parent, mm_select_sub, mm_est_err,
//     mm_filter_strand_retained, mm_set_mapq
// Canonical tie-breaks T1-T4 are those of oracle/mm_oracle.c.
#include "mm_stages.hpp"

#include <algorithm>
#include <atomic>
#include <type_traits>
#include <utility>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

struct hymet_mm_result {
    int n_q = 0;
    std::vector<int64_t> reg_off;   // n_q + 1
    std::vector<int32_t> rep_len;   // n_q
    std::vector<hymet_mm_reg> regs;
};

namespace hymet {
namespace mm {

int launch_regions(hymet_ctx *ctx, const uint64_t *ax, const uint32_t *ax32, const uint32_t *ay, int span, const int32_t *ids,
                   const int64_t *cfirst, const uint64_t *cu, const int64_t *cboff,
                   const int64_t *qc, const int64_t *qb, const int64_t *mp_off, const int64_t *qlen,
                   const uint32_t *name_hash, const int32_t *rep_len, const int64_t *ref_len, int n_q, const hymet_mm_opt *o,
                   int k, void *z, hymet_mm_reg *regs, int32_t *w, uint64_t *cov, int32_t *tmp, int32_t *n_regs,
                   int64_t NB, int64_t NC, const uint32_t *cq,
                   const MiniWord *mtab, const int64_t *qbase, const uint32_t *skip_q);

namespace {

// qid[i] = query of entry i; also ones[i] = 1 (i < n) and zq[q] = 0 (q < n_q) when given
// (grid: max(n, n_q) threads)
__global__ void fill_qid_kernel(const int64_t *off, int n_q, int64_t n, uint32_t *qid, uint32_t *ones, int32_t *zq) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        qid[i] = (uint32_t)upper_idx(off, n_q, i);
        if (ones) ones[i] = 1u;
    }
    if (zq && i < n_q) zq[i] = 0;
}

// per query: its chain anchors when the long join re-chains it, else 0; entry n_q = 0 (the
// scan's total slot); *any = 1 when some query is flagged (the host zeroes the word first)
__global__ void flagged_len_kernel(const uint32_t *flag, const int64_t *qb, int n_q, uint32_t *cnt, int64_t *any) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > n_q) return;
    if (q == n_q) {
        cnt[q] = 0;
        return;
    }
    const bool f = flag[q] != 0;
    cnt[q] = f ? (uint32_t)(qb[q + 1] - qb[q]) : 0u;
    if (f) *any = 1;
}


// seed.c mm_seed_mz_flt: runs of equal (query, x) in the sorted order
__global__ void mzflt_runs_kernel(const uint32_t *sq, const uint64_t *sx, const uint32_t *sidx, const int64_t *qm_off,
                                  int64_t n, int q_occ_max, float q_occ_frac, uint32_t *keep) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (p > 0 && sq[p] == sq[p - 1] && sx[p] == sx[p - 1]) return;  // not a run start
    int64_t e = p + 1;
    while (e < n && sq[e] == sq[p] && sx[e] == sx[p]) e++;
    const uint32_t q = sq[p];
    const int64_t nq = qm_off[q + 1] - qm_off[q];
    if (nq <= q_occ_max) return;  // mm_seed_mz_flt returns early for this query
    const int32_t cnt = (int32_t)(e - p);
    if (cnt > q_occ_max && (float)cnt > (float)nq * q_occ_frac)
        for (int64_t j = p; j < e; j++) keep[sidx[j]] = 0;
}

// mm_seed_mz_flt screen, one block per query: its minimizers are counted into 4096 LDS
// buckets by hash.  A bucket's count bounds the count of every x in it, so a query whose
// buckets all stay at or below q_occ_max has no run to drop (exactly: the filter needs
// cnt > q_occ_max); the others get cnt[q] = their minimizer count and go to the exact (q, x)
// sort.  Also sets keep = 1 for every minimizer.  Block n_q writes the scan's total slot.
constexpr int kMzBuckets = 4096;
__global__ __launch_bounds__(256) void mzflt_screen_kernel(const uint64_t *mx, const int64_t *qm_off, int n_q, int q_occ_max,
                                                           uint32_t *keep, uint32_t *cnt, int64_t *any) {
    __shared__ uint32_t h[kMzBuckets];
    __shared__ int hit;
    const int q = blockIdx.x;
    if (q == n_q) {
        if (threadIdx.x == 0) cnt[q] = 0;
        return;
    }
    const int64_t s = qm_off[q], nq = qm_off[q + 1] - s;
    for (int64_t e = threadIdx.x; e < nq; e += 256) keep[s + e] = 1u;
    if (nq <= q_occ_max) {  // mm_seed_mz_flt returns early for this query
        if (threadIdx.x == 0) cnt[q] = 0;
        return;
    }
    for (int b = threadIdx.x; b < kMzBuckets; b += 256) h[b] = 0;
    if (threadIdx.x == 0) hit = 0;
    __syncthreads();
    bool over = false;
    for (int64_t e = threadIdx.x; e < nq; e += 256)
        over |= atomicAdd(&h[(uint32_t)(mx[s + e] >> 8) & (kMzBuckets - 1)], 1u) >= (uint32_t)q_occ_max;
    if (over) hit = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt[q] = hit ? (uint32_t)nq : 0u;
        if (hit) *any = 1;
    }
}

// the flagged queries' minimizers as one list: global index and query per list entry
__global__ __launch_bounds__(256) void mzflt_list_kernel(const int64_t *qm_off, const uint32_t *cnt, const int64_t *coff,
                                                         uint32_t *gidx, uint32_t *sq) {
    const int q = blockIdx.x;
    const uint32_t nq = cnt[q];
    if (nq == 0) return;
    const int64_t s = qm_off[q], d = coff[q];
    for (uint32_t e = threadIdx.x; e < nq; e += 256) {
        gidx[d + e] = (uint32_t)(s + e);
        sq[d + e] = (uint32_t)q;
    }
}

// out[i] = src[idx[i]] as u64 (x of a list entry) and gout[i] = gidx[perm[i]]
__global__ void mzflt_gather_kernel(const uint32_t *perm, const uint32_t *gidx, const uint64_t *mx, uint32_t *gout,
                                    uint64_t *xout, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = gidx[perm[i]];
    gout[i] = g;
    xout[i] = mx[g];
}

// (also completes the exclusive scan: pos[n] = the kept total)
__global__ void compact_mz_kernel(const uint64_t *x, const uint64_t *y, const uint32_t *keep, int64_t *pos, int64_t n,
                                  uint64_t *ox, uint64_t *oy) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == n - 1) pos[n] = pos[i] + keep[i];
    if (i < n && keep[i]) {
        ox[pos[i]] = x[i];
        oy[pos[i]] = y[i];
    }
}

__global__ void sample_off_kernel(const int64_t *pos, const int64_t *qm_off, int n_q, int64_t total, int64_t *out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > n_q) return;
    out[q] = q == n_q ? total : pos[qm_off[q]];
}

// occurrences of every minimizer (one thread each)
__global__ void seed_count_kernel(const uint64_t *mx, int64_t n, const uint32_t *koff, int64_t n_buckets,
                                  uint32_t *seed_n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t h = mx[i] >> 8;
    uint32_t c = 0;
    if ((int64_t)h < n_buckets) c = koff[h + 1] - koff[h];
    seed_n[i] = c;
}

// ---- mm_seed_select + mm_collect_matches (seed.c), flat over the batch's minimizers.
// The sequential per-query loop is decomposed:
//   * every seed is low (n <= max_occ) or high; one scan of packed (low, high) counts ranks
//     them, and the low / high seeds are listed in order;
//   * a streak (maximal run of high seeds) ends at a low seed or at its query's end: one
//     thread per such end selects the streak's mh kept seeds -- the mh smallest (n, seed
//     number) keys, mh = round((pe - ps) / dist) capped at 128 from the bounding low seeds'
//     positions -- and flags the rest (and every seed above max_max_occ) as filtered;
//   * rep_len = sum over filtered seeds of en - max(st, en of the query's previous filtered
//     seed), the union of their spans (ends increase along the query): one max-scan finds
//     each one's predecessor, one integer atomic per seed sums the query.
constexpr uint32_t kFlt = 0x80000000u;  // filtered flag, kept in bit 31 of seed_n (n < 2^31)

__global__ void seed_class_kernel(const uint32_t *seed_n, int64_t M, int max_occ, uint64_t *cls) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > M) return;
    if (i == M) {  // the scan's extra entry: rank[M] = the totals
        cls[M] = 0;
        return;
    }
    const uint32_t n = seed_n[i];
    const bool hi = (int)n > max_occ, lo = n > 0 && !hi;
    cls[i] = (uint64_t)(hi ? 1u : 0u) << 32 | (lo ? 1u : 0u);
}

__global__ void seed_list_kernel(const uint32_t *seed_n, const uint64_t *rank, int64_t M, int max_occ, int32_t *low_idx,
                                 int32_t *high_idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const uint32_t n = seed_n[i];
    if (!n) return;
    if ((int)n > max_occ) high_idx[rank[i] >> 32] = (int32_t)i;
    else low_idx[(uint32_t)rank[i]] = (int32_t)i;
}

struct StreakParams {
    const uint64_t *my;
    const uint32_t *qid;
    const int64_t *qm_off, *qlen;
    const uint64_t *rank;      // exclusive (low, high) counts, M + 1 entries
    const int32_t *low_idx, *high_idx;
    int64_t n_low;
    int n_q;
    int max_occ, max_max_occ, dist;
    uint32_t *seed_n;
    uint32_t *flt_high;        // per high rank: filtered
};

__global__ void streak_kernel(StreakParams P) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P.n_low + P.n_q) return;
    int q;
    int64_t e_idx = -1, p_idx = -1;  // ending low seed, previous low seed (minimizer indices)
    uint64_t re, rp;                 // (low, high) ranks at the streak's end and start
    if (t < P.n_low) {
        e_idx = P.low_idx[t];
        q = (int)P.qid[e_idx];
        re = P.rank[e_idx];
        if (t > 0 && P.qid[P.low_idx[t - 1]] == (uint32_t)q) p_idx = P.low_idx[t - 1];
    } else {
        q = (int)(t - P.n_low);
        re = P.rank[P.qm_off[q + 1]];
        const uint64_t r0 = P.rank[P.qm_off[q]];
        if ((uint32_t)re > (uint32_t)r0) p_idx = P.low_idx[(uint32_t)re - 1];
    }
    rp = p_idx >= 0 ? P.rank[p_idx] : P.rank[P.qm_off[q]];
    const int64_t h0 = (int64_t)(rp >> 32), h1 = (int64_t)(re >> 32);  // the streak's high ranks
    const int cnt = (int)(h1 - h0);
    if (cnt <= 0) return;
    const bool case_a = P.dist > 0 && P.max_max_occ > P.max_occ;
    bool keep_all = false, keep_none = false;
    uint64_t thr = 0;
    if (case_a) {
        const uint64_t rq0 = P.rank[P.qm_off[q]], rq1 = P.rank[P.qm_off[q + 1]];
        const int64_t n_seed = (int64_t)((uint32_t)rq1 - (uint32_t)rq0) + (int64_t)((rq1 >> 32) - (rq0 >> 32));
        if (n_seed <= 1) return;  // seed.c: nothing is filtered for a single seed
        const int32_t ps = p_idx >= 0 ? (int32_t)((uint32_t)P.my[p_idx] >> 1) : 0;
        const int32_t pe = e_idx >= 0 ? (int32_t)((uint32_t)P.my[e_idx] >> 1) : (int32_t)P.qlen[q];
        int32_t mh = (int32_t)((double)(pe - ps) / P.dist + .499);
        if (mh > 128) mh = 128;
        keep_all = mh >= cnt, keep_none = mh <= 0;
        if (!keep_all && !keep_none) {  // the mh-th smallest (n, index) key
            uint64_t lo = 0, hi = ~0ull;
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                int c = 0;
                for (int64_t r = h0; r < h1; r++) {
                    const int32_t a = P.high_idx[r];
                    c += ((uint64_t)P.seed_n[a] << 32 | (uint32_t)a) <= mid;
                }
                if (c >= mh) hi = mid;
                else lo = mid + 1;
            }
            thr = lo;
        }
    }
    for (int64_t r = h0; r < h1; r++) {
        const int32_t a = P.high_idx[r];
        const uint32_t n = P.seed_n[a];
        bool flt = true;  // case B: every seed above max_occ
        if (case_a) {
            const bool chosen = keep_all || (!keep_none && ((uint64_t)n << 32 | (uint32_t)a) <= thr);
            flt = !chosen || (int)n > P.max_max_occ;
        }
        P.flt_high[r] = flt ? 1u : 0u;
    }
}

// previous filtered high seed: inclusive max-scan of (flt ? rank : -1)
__global__ void flt_mark_kernel(const uint32_t *flt_high, int64_t n_high, int32_t *v) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_high) v[r] = flt_high[r] ? (int32_t)r : -1;
}

__global__ void rep_len_kernel(const uint32_t *flt_high, const int32_t *prev_max, const int32_t *high_idx, int64_t n_high,
                               const uint64_t *mx, const uint64_t *my, const uint32_t *qid, int32_t *rep_len,
                               uint32_t *seed_n) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_high || !flt_high[r]) return;
    const int32_t a = high_idx[r];
    const uint32_t q = qid[a];
    const int32_t en = (int32_t)((uint32_t)my[a] >> 1) + 1, st = en - (int32_t)(mx[a] & 0xff);
    int32_t en_prev = 0;
    const int32_t pr = r > 0 ? prev_max[r - 1] : -1;
    if (pr >= 0) {
        const int32_t b = high_idx[pr];
        if (qid[b] == q) en_prev = (int32_t)((uint32_t)my[b] >> 1) + 1;
    }
    atomicAdd(rep_len + q, en - max(st, en_prev));
    seed_n[a] = 0;  // filtered: not a seed any more
}

__global__ void nz_flag_kernel(const uint32_t *v, int64_t n, uint32_t *flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = v[i] ? 1u : 0u;
}

struct AnchorParams {
    const uint64_t *mx, *my;
    const uint32_t *seed_n;
    const int64_t *a_pos;     // anchor offset of every minimizer
    const uint32_t *qid;
    const int64_t *qlen;
    const uint32_t *koff;
    const uint64_t *ipos;
    int64_t n;
    int rb;                   // bits for rid
    uint64_t *ax, *k1, *k2;
    uint32_t *ay;             // y's low word (the span is idx->k for every minimizer)
    uint32_t *val;
    // mini_pos
    const int64_t *mp_pos;
    uint64_t *mini_pos;
};

__global__ void write_anchors_kernel(AnchorParams P) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t n = P.seed_n[i];
    if (!n) return;
    const uint64_t mx = P.mx[i], my = P.my[i];
    const uint32_t q_pos = (uint32_t)my, q_span = (uint32_t)(mx & 0xff);
    P.mini_pos[P.mp_pos[i]] = (uint64_t)q_span << 32 | (q_pos >> 1);
    const uint32_t q = P.qid[i];
    const int32_t qlen = (int32_t)P.qlen[q];
    const uint32_t *kp = P.koff + (mx >> 8);
    const uint64_t *r = P.ipos + kp[0];
    int64_t a = P.a_pos[i];
    for (uint32_t k = 0; k < n; k++, a++) {
        const uint64_t rk = r[k];
        const uint32_t rpos = (uint32_t)rk >> 1;
        const uint32_t rid = (uint32_t)(rk >> 32);
        uint64_t x, y;
        uint32_t rev;
        if ((rk & 1) == (q_pos & 1)) {
            rev = 0;
            x = (rk & 0xffffffff00000000ULL) | rpos;
            y = (uint64_t)q_span << 32 | (q_pos >> 1);
        } else {
            rev = 1;
            x = 1ULL << 63 | (rk & 0xffffffff00000000ULL) | rpos;
            y = (uint64_t)q_span << 32 | (uint32_t)(qlen - (int32_t)((q_pos >> 1) + 1 - q_span) - 1);
        }
        P.ax[a] = x;
        P.ay[a] = (uint32_t)y;
        P.k1[a] = (uint64_t)q << (1 + P.rb) | (uint64_t)rev << P.rb | rid;
        P.k2[a] = (uint64_t)rpos << 32 | (uint32_t)y;
        P.val[a] = (uint32_t)a;
    }
}

// Anchor words (the default path): one 64-bit word per anchor packing exactly its sort order
// inside its query -- W = (rev | rid | rpos) << ybits | y's low word, field widths from the
// batch (index sequences, longest index sequence, longest query; anchor_word_ybits) -- for
// the grouped sort, which takes the query from the anchor offsets.  A layout without a word
// (ybits == 0) takes write_anchors_kernel and the two-key sort instead.
// The high bits of y hold the span, which is k for every minimizer of a non-HPC sketch.  One
// block per 256 consecutive minimizers: the block stages their anchor offsets, position-list
// starts and query coordinates in LDS, then its 256 lanes sweep the block's anchors
// (contiguous in both the position lists and the output), finding each anchor's minimizer
// by binary search in LDS -- coalesced reads and writes where a lane per minimizer would
// write 20-60 scattered anchors.
struct AnchorKeyParams {
    const uint64_t *mx, *my;
    const uint32_t *seed_n;
    const int64_t *a_pos;     // anchor offset of every minimizer (M + 1 entries)
    const uint32_t *qid;
    const int64_t *qlen;
    const uint32_t *koff;
    const uint64_t *ipos;
    int64_t n;                // minimizers
    int rb, pb;               // bits for rid / rpos
    int ybits;                // bits for y's low word (> 0)
    uint64_t *key;
    const int64_t *mp_pos;
    uint64_t *mini_pos;
};

__global__ __launch_bounds__(256) void write_anchor_keys_kernel(AnchorKeyParams P) {
    __shared__ int64_t s_a[257];
    __shared__ uint64_t s_r[256];   // start of the minimizer's position list
    __shared__ uint32_t s_yf[256], s_yr[256], s_strand[256];
    const int tid = threadIdx.x;
    const int64_t m0 = (int64_t)blockIdx.x * 256;
    const int cnt = (int)min((int64_t)256, P.n - m0);
    if (tid < cnt) {
        const int64_t i = m0 + tid;
        const uint32_t n = P.seed_n[i];
        const uint64_t mx = P.mx[i], my = P.my[i];
        const uint32_t q_pos = (uint32_t)my, q_span = (uint32_t)(mx & 0xff);
        const uint32_t q = P.qid[i];
        if (n) P.mini_pos[P.mp_pos[i]] = (uint64_t)q_span << 32 | (q_pos >> 1);
        s_a[tid] = P.a_pos[i];
        s_r[tid] = P.koff[mx >> 8];
        s_yf[tid] = q_pos >> 1;
        s_yr[tid] = (uint32_t)((int32_t)P.qlen[q] - (int32_t)((q_pos >> 1) + 1 - q_span) - 1);
        s_strand[tid] = q_pos & 1;
    }
    if (tid == 0) s_a[cnt] = P.a_pos[m0 + cnt];
    __syncthreads();
    const int64_t a0 = s_a[0], a1 = s_a[cnt];
    const int sh_rev = P.rb + P.pb;
    for (int64_t a = a0 + tid; a < a1; a += 256) {
        int lo = 0, hi = cnt - 1;  // last s with s_a[s] <= a (its list is non-empty)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_a[mid] <= a) lo = mid;
            else hi = mid - 1;
        }
        const uint64_t rk = P.ipos[s_r[lo] + (a - s_a[lo])];
        const uint32_t rpos = (uint32_t)rk >> 1;
        const uint64_t rid = rk >> 32;
        const uint32_t rev = ((uint32_t)rk & 1) != s_strand[lo];
        const uint64_t k = (uint64_t)rev << sh_rev | rid << P.pb | rpos;
        const uint32_t y = rev ? s_yr[lo] : s_yf[lo];
        P.key[a] = k << P.ybits | y;
    }
}

// query position -> index among the query's seeded minimizers (mini_pos order), for
// mm_est_err's get_mini_idx (MiniWord): pass 1 sets the start bits, pass 2 writes each word's
// base (every seeded minimizer of the word writes the same value: its index less the start
// bits below it)
__global__ __launch_bounds__(256) void mini_bits_kernel(const uint64_t *my, const uint32_t *seed_n, const uint32_t *qid,
                                                        const int64_t *qbase, int64_t M, MiniWord *tab) {
    // consecutive minimizers of a query share words: the bits of a run of lanes on one word
    // are OR-ed across the run and set by one atomic (device-scope atomics are the costly part)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool on = i < M && seed_n[i];
    const int64_t b = on ? qbase[qid[i]] + ((uint32_t)my[i] >> 1) : -64 * (int64_t)(lane + 1);  // distinct dummy words
    const int64_t w = b >> 6;
    uint64_t bits = on ? 1ull << (b & 63) : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {  // OR over the lanes of the same word (runs are contiguous)
        const int64_t wo = __shfl_down(w, d, 64);
        const uint64_t bo = __shfl_down(bits, d, 64);
        if (lane + d < 64 && wo == w) bits |= bo;
    }
    const int64_t wp = __shfl_up(w, 1, 64);
    if (on && (lane == 0 || wp != w)) atomicOr((unsigned long long *)&tab[w].bits, bits);
}
__global__ void mini_base_kernel(const uint64_t *my, const uint32_t *seed_n, const uint32_t *qid, const int64_t *qm_off,
                                 const int64_t *mp_pos, const int64_t *qbase, int64_t M, MiniWord *tab) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M || !seed_n[i]) return;
    const uint32_t q = qid[i];
    const int64_t b = qbase[q] + ((uint32_t)my[i] >> 1);
    const uint64_t bits = tab[b >> 6].bits;
    tab[b >> 6].base = (uint32_t)(mp_pos[i] - mp_pos[qm_off[q]]) - (uint32_t)__popcll(bits & ((1ull << (b & 63)) - 1));
}

// per query: regions kept (first-pass chains, or the long-join re-chain's for flagged queries)
__global__ void reg_count_kernel(const uint32_t *flag, const int32_t *n1, const int32_t *n2, int n_q, uint32_t *cnt) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n_q) cnt[q] = (uint32_t)((flag && flag[q]) ? n2[q] : n1[q]);
}

// one thread per query: copy its region records to their PAF positions (+ line metadata)
struct RegOut {
    hymet_mm_reg *regs;
    int32_t *q, *part, *rl, *t;  // optional (accumulator sink)
    int32_t q_base, part_id, t_base;
};
__global__ void reg_gather_kernel(const uint32_t *flag, const int32_t *n1, const int32_t *n2, const int64_t *qc1,
                                  const int64_t *qc2, const hymet_mm_reg *r1, const hymet_mm_reg *r2, const int64_t *off,
                                  const int32_t *rep_len, int n_q, RegOut o) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    const bool use2 = flag && flag[q];
    const hymet_mm_reg *src = use2 ? r2 + qc2[q] : r1 + qc1[q];
    const int nr = use2 ? n2[q] : n1[q];
    const int64_t d = off[q];
    for (int i = 0; i < nr; i++) {
        const hymet_mm_reg r = src[i];
        o.regs[d + i] = r;
        if (o.q) {
            o.q[d + i] = o.q_base + q;
            o.part[d + i] = o.part_id;
            o.rl[d + i] = rep_len[q];
            o.t[d + i] = o.t_base + r.rid;
        }
    }
}
}  // namespace
}  // namespace mm
}  // namespace hymet

using namespace hymet;
using namespace hymet::mm;

// ---------------------------------------------------------------- host helpers
// HYMET_TRACE=1: whole-call wall time of hymet_mm_map, destructors included
struct CallTrace {
    bool on = env_flag("HYMET_TRACE");
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    ~CallTrace() {
        if (on)
            fprintf(stderr, "[hymet_mm_map] %-22s %9.2f ms\n", "TOTAL (with frees)",
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count());
    }
};
// HYMET_TRACE=1: per-phase wall times of hymet_mm_map (stream synchronised at each mark)
struct PhaseTrace {
    hymet_ctx *ctx;
    bool on;
    std::chrono::steady_clock::time_point t;
    explicit PhaseTrace(hymet_ctx *c) : ctx(c), on(env_flag("HYMET_TRACE")), t(std::chrono::steady_clock::now()) {}
    void mark(const char *what) {
        if (!on) return;
        (void)hipStreamSynchronize(ctx->stream);
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "[hymet_mm_map] %-22s %9.2f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

// the two-key fallback (layouts without a word, HYMET_ANCHOR_LEGACY=1): sort raw anchors (x,
// y's low word, k1 with k2 keys) into an AnchorSet -- by (tpos, qpos), then stably by (query,
// strand, target) -- through a permutation, with the library's LSD radix sort
static int sort_anchor_set(hymet_ctx *ctx, DevBuf &x, DevBuf &y, DevBuf &k1, DevBuf &k2, DevBuf &val, int64_t n,
                           int key1_bits, int yhi, AnchorSet &out) {
    DevBuf k2b, valb, k1g, k1b;
    HY_HIP(k2b.alloc(8 * (size_t)n, ctx->stream));
    HY_HIP(valb.alloc(4 * (size_t)n, ctx->stream));
    uint64_t *kk = k2.as<uint64_t>(), *kka = k2b.as<uint64_t>();
    uint32_t *vv = val.as<uint32_t>(), *vva = valb.as<uint32_t>();
    int rc = sort_pairs(ctx, kk, kka, vv, vva, n, 0, 64, "radix_sort_anchor_pos");
    if (rc) return rc;
    HY_HIP(k1g.alloc(8 * (size_t)n, ctx->stream));
    HY_HIP(k1b.alloc(8 * (size_t)n, ctx->stream));
    LAUNCH1(gather_kernel<uint64_t>, n, k1.as<uint64_t>(), vv, k1g.as<uint64_t>(), n);
    uint64_t *k1p = k1g.as<uint64_t>(), *k1a = k1b.as<uint64_t>();
    rc = sort_pairs(ctx, k1p, k1a, vv, vva, n, 0, key1_bits, "radix_sort_anchor_group");
    if (rc) return rc;
    HY_HIP(out.ax.alloc(8 * (size_t)n, ctx->stream));
    HY_HIP(out.ay.alloc(4 * (size_t)n, ctx->stream));
    LAUNCH1(gather_kernel<uint64_t>, n, x.as<uint64_t>(), vv, out.ax.as<uint64_t>(), n);
    LAUNCH1(gather_kernel<uint32_t>, n, y.as<uint32_t>(), vv, out.ay.as<uint32_t>(), n);
    out.n = n;
    out.span = yhi & 0xff;
    return HYMET_OK;
}

// sort anchor words (write_anchor_keys_kernel) into an AnchorSet: the per-query grouped sort
// (mm_asort.hip), which writes (x, y) itself
static int sort_anchor_words(hymet_ctx *ctx, DevBuf &word, int64_t n, int rb, int pb, int yhi, const int64_t *d_qoff, int n_q,
                             int64_t max_qlen, AnchorSet &out) {
    DevBuf wb;
    HY_HIP(wb.alloc(8 * (size_t)n, ctx->stream));
    HY_HIP(out.ax.alloc(8 * (size_t)n, ctx->stream));
    HY_HIP(out.ay.alloc(4 * (size_t)n, ctx->stream));
    HY_HIP(out.hb.alloc(head_bits_bytes(n), ctx->stream));
    HY_HIP(out.ax32.alloc(4 * (size_t)n, ctx->stream));
    out.n = n;
    out.span = yhi & 0xff;
    // HYMET_ASORT_STATS=1: every batch's block-sort counts on stderr (a measuring aid: it
    // adds a stream synchronise per batch) -- segments and anchors finished by the outlier
    // path, segments and anchors that took the full sort
    const bool log_stats = env_flag("HYMET_ASORT_STATS");
    DevBuf sstat;
    if (log_stats) {
        HY_HIP(sstat.alloc(32, ctx->stream));
        HY_HIP(hipMemsetAsync(sstat.p, 0, 32, ctx->stream));
    }
    const int rc = grouped_anchor_sort(ctx, word.as<uint64_t>(), n, d_qoff, n_q, rb, pb, max_qlen,
                                       wb.as<uint64_t>(), out.ax.as<uint64_t>(), out.ay.as<uint32_t>(),
                                       out.hb.as<uint32_t>(), out.ax32.as<uint32_t>(),
                                       log_stats ? sstat.as<unsigned long long>() : nullptr);
    if (rc == 1) return hymet::fail(HYMET_E_INTERNAL, "sort_anchor_words: anchor words emitted for a layout without one");
    if (rc) return rc;
    if (log_stats) {
        unsigned long long h[4] = {};
        HY_HIP(hipMemcpyAsync(h, sstat.p, 32, hipMemcpyDeviceToHost, ctx->stream));
        HY_HIP(hipStreamSynchronize(ctx->stream));
        fprintf(stderr, "[asort] anchors %lld fast_segs %llu fast_anchors %llu full_segs %llu full_anchors %llu\n",
                (long long)n, h[0], h[1], h[2], h[3]);
    }
    out.has_hb = out.has_x32 = true;
    return HYMET_OK;
}

// HYMET_DUMP_ANCHORS=path (profiling, tools/chain_prof): the first call's sorted first-pass
// anchors as (x, y) pairs with x>>32 replaced by the (query, strand, target) group ordinal;
// HYMET_DUMP_ANCHORS2=path: the same for the long-join re-chain's anchors.  `dumped`: the
// variable's one dump of the process has been claimed (the mapping threads share the flag).
static int dump_anchors(hymet_ctx *ctx, const char *var, const AnchorSet &S, int n_q, std::atomic<bool> &dumped) {
    const char *path = env_str(var);
    if (!path || S.n == 0 || dumped.exchange(true)) return HYMET_OK;
    hipStream_t st = ctx->stream;
    const int64_t nd = std::min<int64_t>(S.n, env_int("HYMET_DUMP_MAX", 1 << 24, 0, INT64_MAX));  // anchors to dump
    std::vector<uint64_t> hx(nd);
    std::vector<uint32_t> hy(nd);  // widened with the set's span on the way out
    std::vector<int64_t> qo(n_q + 1);
    HY_HIP(hipMemcpyAsync(hx.data(), S.ax.p, 8 * (size_t)nd, hipMemcpyDeviceToHost, st));
    HY_HIP(hipMemcpyAsync(hy.data(), S.ay.p, 4 * (size_t)nd, hipMemcpyDeviceToHost, st));
    HY_HIP(hipMemcpyAsync(qo.data(), S.d_off.p, 8 * (size_t)(n_q + 1), hipMemcpyDeviceToHost, st));
    HY_HIP(hipStreamSynchronize(st));
    if (FILE *fp = fopen(path, "wb")) {
        uint64_t gid = 0;
        int q = 0;
        std::vector<uint64_t> buf;
        buf.reserve(1 << 21);
        for (int64_t a = 0; a < nd; a++) {
            bool qs = false;  // a query's first anchor
            while (q < n_q && qo[q + 1] <= a) q++, qs = true;
            if (a && (qs || (hx[a] >> 32) != (hx[a - 1] >> 32))) gid++;
            buf.push_back(gid << 32 | (uint32_t)hx[a]);
            buf.push_back((uint64_t)S.span << 32 | hy[a]);
            if (buf.size() >= (1u << 21)) fwrite(buf.data(), 8, buf.size(), fp), buf.clear();
        }
        fwrite(buf.data(), 8, buf.size(), fp);
        fclose(fp);
    }
    return HYMET_OK;
}

// where hymet_mm_map puts a batch's PAF records: host vectors (hymet_mm_result) or the
// device-resident accumulator of a run (hymet_paf_acc)
struct MapSink {
    hymet_mm_result *res = nullptr;
    hymet_paf_acc *acc = nullptr;
    int32_t q_base = 0, part_id = 0, t_base = 0;
};

static int acc_reserve(hymet_ctx *ctx, hymet_paf_acc *a, int64_t need) {
    if (need <= a->cap) return HYMET_OK;
    const int64_t cap = std::max<int64_t>(need, std::max<int64_t>(a->cap * 3 / 2, 1 << 16));
    hipStream_t st = ctx->stream;
    DevBuf nregs, nq, npart, nrl, nt;
    HY_HIP(nregs.alloc(sizeof(hymet_mm_reg) * (size_t)cap, st));
    HY_HIP(nq.alloc(4 * (size_t)cap, st));
    HY_HIP(npart.alloc(4 * (size_t)cap, st));
    HY_HIP(nrl.alloc(4 * (size_t)cap, st));
    HY_HIP(nt.alloc(4 * (size_t)cap, st));
    if (a->n) {
        HY_HIP(hipMemcpyAsync(nregs.p, a->regs.p, sizeof(hymet_mm_reg) * (size_t)a->n, hipMemcpyDeviceToDevice, st));
        HY_HIP(hipMemcpyAsync(nq.p, a->q.p, 4 * (size_t)a->n, hipMemcpyDeviceToDevice, st));
        HY_HIP(hipMemcpyAsync(npart.p, a->part.p, 4 * (size_t)a->n, hipMemcpyDeviceToDevice, st));
        HY_HIP(hipMemcpyAsync(nrl.p, a->rl.p, 4 * (size_t)a->n, hipMemcpyDeviceToDevice, st));
        HY_HIP(hipMemcpyAsync(nt.p, a->t.p, 4 * (size_t)a->n, hipMemcpyDeviceToDevice, st));
    }
    a->regs.swap(nregs);
    a->q.swap(nq);
    a->part.swap(npart);
    a->rl.swap(nrl);
    a->t.swap(nt);
    a->cap = cap;
    return HYMET_OK;
}

// ---------------------------------------------------------------- stages of hymet_mm_map
// What the stages of one call share: the call's arguments and the device buffers that more
// than one stage reads.  All of it lives until the call returns; a stage's own temporaries
// are released when the stage does.
struct MapBatch {
    hymet_ctx *ctx;
    const hymet_mm_index *idx;
    const hymet_mm_opt *opt;
    const int64_t *h_lens;
    int32_t n_q;
    DevBuf mx, my, qm_off;  // the queries' minimizers (query-major) and n_q + 1 offsets into them
    int64_t M = 0;
    DevBuf d_qlen, d_hash_buf;
    const uint32_t *d_hash = nullptr;  // query name hashes: the caller's device copy, or d_hash_buf
    DevBuf seed_n, rep_len, qid;       // per minimizer: seed count (| kFlt), query; per query: rep_len
    DevBuf mini_pos, mp_off;           // the seeded minimizers' positions (NM) and n_q + 1 offsets
    int64_t NM = 0;
    // mm_est_err's minimizer lookup table: each query's bases at a 64-aligned offset, 16 B per 64 bases
    DevBuf d_qbase, pos_tab;
    std::vector<int64_t> qbase;  // lives until the call returns (async H2D source)
    int64_t max_qlen = 1;
};

// 1 sketch: the queries' minimizers, lengths and name hashes on the device
static int sketch_queries(MapBatch &B, const uint32_t *d_2b, const uint32_t *d_mask, const int64_t *h_starts,
                          const uint32_t *h_name_hash, const uint32_t *d_name_hash) {
    hipStream_t st = B.ctx->stream;
    const int n_q = B.n_q;
    int rc = sketch_sequences(B.ctx, d_2b, d_mask, h_starts, B.h_lens, n_q, B.idx->w, B.idx->k, 0, B.mx, B.my, &B.M, &B.qm_off);
    if (rc) return rc;
    HY_HIP(B.d_qlen.alloc(8 * (size_t)n_q, st));
    HY_HIP(hipMemcpyAsync(B.d_qlen.p, B.h_lens, 8 * (size_t)n_q, hipMemcpyHostToDevice, st));
    B.d_hash = d_name_hash;  // the caller's device copy when it has one
    if (!B.d_hash) {
        HY_HIP(B.d_hash_buf.alloc(4 * (size_t)n_q, st));
        HY_HIP(hipMemcpyAsync(B.d_hash_buf.p, h_name_hash, 4 * (size_t)n_q, hipMemcpyHostToDevice, st));
        B.d_hash = B.d_hash_buf.as<uint32_t>();
    }
    return HYMET_OK;
}

// 2 mm_seed_mz_flt: drops each query's over-represented minimizers from mx / my / qm_off.
// Only queries with more than mid_occ minimizers are filtered: an LDS bucket screen clears
// most of them, the exact filter runs over the minimizers of the others.
static int filter_minimizers(MapBatch &B) {
    hymet_ctx *ctx = B.ctx;
    hipStream_t st = ctx->stream;
    const hymet_mm_opt *opt = B.opt;
    const int n_q = B.n_q;
    const int64_t M = B.M;
    DevBuf &mx = B.mx, &my = B.my, &qm_off = B.qm_off;
    DevBuf keep, fcnt, fcoff;
    int64_t MF = 0;  // minimizers of the queries the screen could not clear
    int rc;
    if (opt->q_occ_frac > 0.0f && M > 0 && opt->mid_occ > 0) {
        HY_HIP(keep.alloc(4 * (size_t)M, st));
        HY_HIP(fcnt.alloc(4 * (size_t)(n_q + 1), st));
        ctx->mbox_h[kMbFlag] = 0;
        hipLaunchKernelGGL(mzflt_screen_kernel, dim3((unsigned)n_q + 1), dim3(256), 0, st, mx.as<uint64_t>(), qm_off.as<int64_t>(),
                           n_q, opt->mid_occ, keep.as<uint32_t>(), fcnt.as<uint32_t>(), mb_dev(ctx, kMbFlag));
        HY_CHECK_LAUNCH("mzflt_screen_kernel");
        HY_HIP(hipStreamSynchronize(st));
        if (mb_read(ctx, kMbFlag) != 0) {
            HY_HIP(fcoff.alloc(8 * (size_t)(n_q + 1), st));
            rc = exclusive_scan_u32_i64(ctx, fcnt.as<uint32_t>(), fcoff.as<int64_t>(), n_q + 1, &MF);
            if (rc) return rc;
        }
    }
    if (MF == 0) return HYMET_OK;
    // the exact filter over the flagged queries' minimizers only: list entries sorted by x,
    // then stably by query, runs of equal (q, x) counted
    DevBuf gidx, sx, sx2, sidx, sidx2, sq0, sq, sq2, kpos, nx, ny, gx, gg;
    HY_HIP(gidx.alloc(4 * (size_t)MF, st));
    HY_HIP(sq0.alloc(4 * (size_t)MF, st));
    hipLaunchKernelGGL(mzflt_list_kernel, dim3((unsigned)n_q), dim3(256), 0, st, qm_off.as<int64_t>(), fcnt.as<uint32_t>(),
                       fcoff.as<int64_t>(), gidx.as<uint32_t>(), sq0.as<uint32_t>());
    HY_CHECK_LAUNCH("mzflt_list_kernel");
    HY_HIP(sx.alloc(8 * (size_t)MF, st));
    HY_HIP(sx2.alloc(8 * (size_t)MF, st));
    HY_HIP(sidx.alloc(4 * (size_t)MF, st));
    HY_HIP(sidx2.alloc(4 * (size_t)MF, st));
    LAUNCH1(gather_kernel<uint64_t>, MF, mx.as<uint64_t>(), gidx.as<uint32_t>(), sx.as<uint64_t>(), MF);
    LAUNCH1(iota_u32_kernel, MF, sidx.as<uint32_t>(), MF);
    uint64_t *kx = sx.as<uint64_t>(), *kxa = sx2.as<uint64_t>();
    uint32_t *vi = sidx.as<uint32_t>(), *via = sidx2.as<uint32_t>();
    rc = sort_pairs(ctx, kx, kxa, vi, via, MF, 0, 2 * B.idx->k + 8, "radix_sort_mz");
    if (rc) return rc;
    HY_HIP(sq.alloc(4 * (size_t)MF, st));
    HY_HIP(sq2.alloc(4 * (size_t)MF, st));
    LAUNCH1(gather_kernel<uint32_t>, MF, sq0.as<uint32_t>(), vi, sq.as<uint32_t>(), MF);
    uint32_t *kq = sq.as<uint32_t>(), *kqa = sq2.as<uint32_t>();
    rc = sort_pairs(ctx, kq, kqa, vi, via, MF, 0, bits_for(n_q), "radix_sort_mz");
    if (rc) return rc;
    HY_HIP(gx.alloc(8 * (size_t)MF, st));
    HY_HIP(gg.alloc(4 * (size_t)MF, st));
    LAUNCH1(mzflt_gather_kernel, MF, vi, gidx.as<uint32_t>(), mx.as<uint64_t>(), gg.as<uint32_t>(), gx.as<uint64_t>(), MF);
    LAUNCH1(mzflt_runs_kernel, MF, kq, gx.as<uint64_t>(), gg.as<uint32_t>(), qm_off.as<int64_t>(), MF, opt->mid_occ,
            opt->q_occ_frac, keep.as<uint32_t>());
    int64_t M2 = 0;
    rc = scan_flags(ctx, keep.as<uint32_t>(), M, kpos, &M2);
    if (rc) return rc;
    HY_HIP(nx.alloc(8 * (size_t)(M2 + 1), st));
    HY_HIP(ny.alloc(8 * (size_t)(M2 + 1), st));
    LAUNCH1(compact_mz_kernel, M, mx.as<uint64_t>(), my.as<uint64_t>(), keep.as<uint32_t>(), kpos.as<int64_t>(), M,
            nx.as<uint64_t>(), ny.as<uint64_t>());
    DevBuf nqm;
    HY_HIP(nqm.alloc(8 * (size_t)(n_q + 1), st));
    hipLaunchKernelGGL(sample_off_kernel, dim3((unsigned)cdiv(n_q + 1, 256)), dim3(256), 0, st, kpos.as<int64_t>(),
                       qm_off.as<int64_t>(), n_q, M2, nqm.as<int64_t>());
    HY_CHECK_LAUNCH("sample_off_kernel");
    mx.swap(nx);
    my.swap(ny);
    qm_off.swap(nqm);
    B.M = M2;
    return HYMET_OK;
}

// 3 seeds: every minimizer's occurrence count (seed_n, kFlt where mm_seed_select drops it),
// its query (qid) and each query's rep_len
static int select_seeds(MapBatch &B) {
    hymet_ctx *ctx = B.ctx;
    hipStream_t st = ctx->stream;
    const hymet_mm_opt *opt = B.opt;
    const int n_q = B.n_q;
    const int64_t M = B.M;
    DevBuf &mx = B.mx, &my = B.my, &qm_off = B.qm_off, &seed_n = B.seed_n, &rep_len = B.rep_len, &qid = B.qid;
    HY_HIP(seed_n.alloc(4 * (size_t)(M + 1), st));
    HY_HIP(rep_len.alloc(4 * (size_t)n_q, st));
    HY_HIP(qid.alloc(4 * (size_t)(M + 1), st));
    LAUNCH1(fill_qid_kernel, std::max<int64_t>(M, n_q), qm_off.as<int64_t>(), n_q, M, qid.as<uint32_t>(), nullptr,
            rep_len.as<int32_t>());
    {
        ProfScope _ps(ctx, "mm_seed_count", (double)M * (8.0 + 8.0 + 4.0));  // minimizer, 2 offsets, count
        LAUNCH1(seed_count_kernel, M, mx.as<uint64_t>(), M, B.idx->d_koff, B.idx->n_buckets, seed_n.as<uint32_t>());
    }
    if (M == 0) return HYMET_OK;
    ProfScope _ps(ctx, "mm_seed_select", (double)M * (4.0 + 8.0 + 8.0 + 8.0));  // count, class, rank, list
    DevBuf cls, rank, spart;
    HY_HIP(cls.alloc(8 * (size_t)(M + 1), st));
    HY_HIP(rank.alloc(8 * (size_t)(M + 1), st));
    LAUNCH1(seed_class_kernel, M + 1, seed_n.as<uint32_t>(), M, opt->mid_occ, cls.as<uint64_t>());
    // exclusive scan of packed (low, high) counts over M + 1 entries: rank[M] = totals
    int rc = scan_u64(ctx, cls.as<uint64_t>(), rank.as<uint64_t>(), M + 1, spart, mb_dev(ctx, kMbScan));
    if (rc) return rc;
    HY_HIP(hipStreamSynchronize(st));
    const uint64_t tot = (uint64_t)mb_read(ctx, kMbScan);
    const int64_t n_low = (uint32_t)tot, n_high = (int64_t)(tot >> 32);
    if (n_high == 0) return HYMET_OK;
    DevBuf low_idx, high_idx, flt_high, vmax, pmax;
    HY_HIP(low_idx.alloc(4 * (size_t)(n_low + 1), st));
    HY_HIP(high_idx.alloc(4 * (size_t)n_high, st));
    HY_HIP(flt_high.alloc(4 * (size_t)n_high, st));
    LAUNCH1(seed_list_kernel, M, seed_n.as<uint32_t>(), rank.as<uint64_t>(), M, opt->mid_occ, low_idx.as<int32_t>(),
            high_idx.as<int32_t>());
    StreakParams S{my.as<uint64_t>(), qid.as<uint32_t>(), qm_off.as<int64_t>(), B.d_qlen.as<int64_t>(),
                   rank.as<uint64_t>(), low_idx.as<int32_t>(), high_idx.as<int32_t>(), n_low, n_q, opt->mid_occ,
                   opt->max_max_occ, opt->occ_dist, seed_n.as<uint32_t>(), flt_high.as<uint32_t>()};
    HY_HIP(hipMemsetAsync(flt_high.p, 0, 4 * (size_t)n_high, st));
    LAUNCH1(streak_kernel, n_low + n_q, S);
    HY_HIP(vmax.alloc(4 * (size_t)n_high, st));
    HY_HIP(pmax.alloc(4 * (size_t)n_high, st));
    LAUNCH1(flt_mark_kernel, n_high, flt_high.as<uint32_t>(), n_high, vmax.as<int32_t>());
    {
        DevBuf mpart;
        rc = inclusive_max_scan_i32(ctx, vmax.as<int32_t>(), pmax.as<int32_t>(), n_high, mpart);
        if (rc) return rc;
    }
    LAUNCH1(rep_len_kernel, n_high, flt_high.as<uint32_t>(), pmax.as<int32_t>(), high_idx.as<int32_t>(), n_high,
            mx.as<uint64_t>(), my.as<uint64_t>(), qid.as<uint32_t>(), rep_len.as<int32_t>(), seed_n.as<uint32_t>());
    return HYMET_OK;
}

// mm_est_err's minimizer lookup table (seed_n is final); also the longest query
static int build_mini_table(MapBatch &B, const DevBuf &mp_pos) {
    hymet_ctx *ctx = B.ctx;
    hipStream_t st = ctx->stream;
    const int n_q = B.n_q;
    B.qbase.assign(n_q + 1, 0);
    for (int q = 0; q < n_q; q++) {
        B.qbase[q + 1] = B.qbase[q] + ((B.h_lens[q] + 63) & ~(int64_t)63);
        B.max_qlen = std::max<int64_t>(B.max_qlen, B.h_lens[q]);
    }
    HY_HIP(B.d_qbase.alloc(8 * (size_t)(n_q + 1), st));
    HY_HIP(hipMemcpyAsync(B.d_qbase.p, B.qbase.data(), 8 * (size_t)(n_q + 1), hipMemcpyHostToDevice, st));
    const size_t n_words = (size_t)(B.qbase[n_q] >> 6) + 1;
    HY_HIP(B.pos_tab.alloc(sizeof(MiniWord) * n_words, st));
    HY_HIP(hipMemsetAsync(B.pos_tab.p, 0, sizeof(MiniWord) * n_words, st));
    LAUNCH1(mini_bits_kernel, B.M, B.my.as<uint64_t>(), B.seed_n.as<uint32_t>(), B.qid.as<uint32_t>(), B.d_qbase.as<int64_t>(),
            B.M, B.pos_tab.as<MiniWord>());
    LAUNCH1(mini_base_kernel, B.M, B.my.as<uint64_t>(), B.seed_n.as<uint32_t>(), B.qid.as<uint32_t>(), B.qm_off.as<int64_t>(),
            mp_pos.as<int64_t>(), B.d_qbase.as<int64_t>(), B.M, B.pos_tab.as<MiniWord>());
    return HYMET_OK;
}

// 4 anchors + 5 sort: one anchor per seed occurrence (and the seeded minimizers' positions,
// mini_pos / mp_off), sorted by (query, strand, target, tpos, qpos) into S1
static int first_pass_anchors(MapBatch &B, AnchorSet &S1) {
    hymet_ctx *ctx = B.ctx;
    hipStream_t st = ctx->stream;
    const hymet_mm_index *idx = B.idx;
    const int n_q = B.n_q;
    const int64_t M = B.M;
    DevBuf &mx = B.mx, &my = B.my, &qm_off = B.qm_off, &seed_n = B.seed_n, &qid = B.qid, &d_qlen = B.d_qlen;
    DevBuf a_pos, mflag, mp_pos;
    int64_t A = 0;
    int rc = scan_flags(ctx, seed_n.as<uint32_t>(), M, a_pos, &A);
    if (rc) return rc;
    HY_ARG(A <= anchor_cap(), "hymet_mm_map: the batch has more anchors than 32-bit chain links hold (map fewer bases per batch)");
    HY_HIP(mflag.alloc(4 * (size_t)(M + 1), st));
    LAUNCH1(nz_flag_kernel, M, seed_n.as<uint32_t>(), M, mflag.as<uint32_t>());
    rc = scan_flags(ctx, mflag.as<uint32_t>(), M, mp_pos, &B.NM);
    if (rc) return rc;
    HY_HIP(hipMemcpyAsync(a_pos.as<int64_t>() + M, &A, 8, hipMemcpyHostToDevice, st));
    HY_HIP(hipMemcpyAsync(mp_pos.as<int64_t>() + M, &B.NM, 8, hipMemcpyHostToDevice, st));
    HY_HIP(B.mini_pos.alloc(8 * (size_t)(B.NM + 1), st));
    HY_HIP(B.mp_off.alloc(8 * (size_t)(n_q + 1), st));
    hipLaunchKernelGGL(sample_off_kernel, dim3((unsigned)cdiv(n_q + 1, 256)), dim3(256), 0, st, mp_pos.as<int64_t>(),
                       qm_off.as<int64_t>(), n_q, B.NM, B.mp_off.as<int64_t>());
    HY_CHECK_LAUNCH("sample_off_kernel");
    rc = build_mini_table(B, mp_pos);
    if (rc) return rc;
    HY_HIP(S1.d_off.alloc(8 * (size_t)(n_q + 1), st));
    hipLaunchKernelGGL(sample_off_kernel, dim3((unsigned)cdiv(n_q + 1, 256)), dim3(256), 0, st, a_pos.as<int64_t>(),
                       qm_off.as<int64_t>(), n_q, A, S1.d_off.as<int64_t>());
    HY_CHECK_LAUNCH("sample_off_kernel");
    // the sort key's fields: bits of the target id and position, of (query, strand, target)
    const int rb = bits_for(idx->n_seq), key1_bits = bits_for(n_q) + 1 + rb;
    HY_ARG(key1_bits <= 64, "hymet_mm_map: too many queries x targets for the sort key");
    int64_t max_len = 1;
    for (int64_t l : idx->h_len) max_len = std::max(max_len, l);
    const int pb = bits_for(max_len - 1);
    if (A == 0) {  // no seed at all: the empty set (n = 0, offsets all zero) on either path
        S1.span = idx->k & 0xff;
        return HYMET_OK;
    }
    // anchors as words for the grouped sort where the batch's layout has one (rb + pb <= 38
    // with queries below 16 Mbp); else the two-key path
    const int ybits = env_flag("HYMET_ANCHOR_LEGACY") ? 0 : anchor_word_ybits(rb, pb, B.max_qlen);
    if (ybits > 0) {
        DevBuf word;
        HY_HIP(word.alloc(8 * (size_t)(A + 1), st));
        AnchorKeyParams P{mx.as<uint64_t>(), my.as<uint64_t>(), seed_n.as<uint32_t>(), a_pos.as<int64_t>(),
                          qid.as<uint32_t>(), d_qlen.as<int64_t>(), idx->d_koff, idx->d_pos, M, rb, pb,
                          ybits, word.as<uint64_t>(), mp_pos.as<int64_t>(), B.mini_pos.as<uint64_t>()};
        {
            // position fetch + word write; the benchmark counts anchors as this scope's bytes
            // / 20, so the constant stays though a word is 8 B where a key and its value were 12
            ProfScope _ps(ctx, "mm_anchors", (double)A * (8.0 + 12.0));
            hipLaunchKernelGGL(write_anchor_keys_kernel, dim3((unsigned)cdiv(M, 256)), dim3(256), 0, st, P);
            HY_CHECK_LAUNCH("write_anchor_keys_kernel");
        }
        return sort_anchor_words(ctx, word, A, rb, pb, idx->k, S1.d_off.as<int64_t>(), n_q, B.max_qlen, S1);
    }
    DevBuf x, y, k1, k2, val;
    HY_HIP(x.alloc(8 * (size_t)(A + 1), st));
    HY_HIP(y.alloc(4 * (size_t)(A + 1), st));
    HY_HIP(k1.alloc(8 * (size_t)(A + 1), st));
    HY_HIP(k2.alloc(8 * (size_t)(A + 1), st));
    HY_HIP(val.alloc(4 * (size_t)(A + 1), st));
    AnchorParams P{mx.as<uint64_t>(), my.as<uint64_t>(), seed_n.as<uint32_t>(), a_pos.as<int64_t>(), qid.as<uint32_t>(),
                   d_qlen.as<int64_t>(), idx->d_koff, idx->d_pos, M, rb, x.as<uint64_t>(), k1.as<uint64_t>(),
                   k2.as<uint64_t>(), y.as<uint32_t>(), val.as<uint32_t>(), mp_pos.as<int64_t>(), B.mini_pos.as<uint64_t>()};
    ProfScope _ps(ctx, "mm_anchors", (double)A * (8.0 + 36.0));  // position fetch + anchor/key writes
    LAUNCH1(write_anchors_kernel, M, P);
    return sort_anchor_set(ctx, x, y, k1, k2, val, A, key1_bits, idx->k, S1);
}

// 7 long join, its anchor set: the chain anchors of the queries the first pass flagged
// (`flag`), compacted out of the first-pass set S1 -- which keeps its (query, x, y) order --
// into S2; any: some query is flagged
static int long_join_anchors(MapBatch &B, const AnchorSet &S1, const LeanJoin &lj, const DevBuf &flag, AnchorSet &S2,
                             bool &any) {
    hymet_ctx *ctx = B.ctx;
    const int n_q = B.n_q;
    // anchors of flagged queries only: their per-query offsets, built on the device (the
    // total and whether any query is flagged come back through the mailbox)
    DevBuf fcnt;
    HY_HIP(fcnt.alloc(4 * (size_t)(n_q + 1), ctx->stream));
    ctx->mbox_h[kMbFlag] = 0;
    LAUNCH1(flagged_len_kernel, n_q + 1, flag.as<uint32_t>(), lj.qb2.as<int64_t>(), n_q, fcnt.as<uint32_t>(),
            mb_dev(ctx, kMbFlag));
    int64_t A2 = 0;
    int rc = scan_flags(ctx, fcnt.as<uint32_t>(), n_q + 1, S2.d_off, &A2);  // (syncs the stream)
    if (rc) return rc;
    any = mb_read(ctx, kMbFlag) != 0;
    if (!any) return HYMET_OK;
    HY_ARG(A2 <= anchor_cap(), "hymet_mm_map: the long join has more anchors than 32-bit chain links hold");
    // their chain anchors carry mark 2 from the backtrack
    rc = marked_anchor_set(ctx, S1, lj, flag.as<uint32_t>(), n_q, A2, S2);
    if (rc) return rc;
    static std::atomic<bool> dumped{false};
    return dump_anchors(ctx, "HYMET_DUMP_ANCHORS2", S2, n_q, dumped);
}

// 8 regions of one chain set: records at the set's chain offsets (rg) + per-query counts (nr)
static int run_regions(MapBatch &B, ChainSet &C, DevBuf &rg, DevBuf &nr, const uint32_t *skip_q) {
    hipStream_t st = B.ctx->stream;
    const int64_t NC = C.n_chain;
    DevBuf z, wv, cov, tmp;
    HY_HIP(z.alloc(16 * (size_t)(NC + 1), st));
    HY_HIP(rg.alloc(sizeof(hymet_mm_reg) * (size_t)(NC + 1), st));
    HY_HIP(wv.alloc(4 * (size_t)(NC + 1), st));
    HY_HIP(cov.alloc(8 * (size_t)(NC + 1), st));
    HY_HIP(tmp.alloc(4 * (size_t)(NC + 1), st));
    HY_HIP(nr.alloc(4 * (size_t)B.n_q, st));
    return launch_regions(B.ctx, C.ax, C.ax32, C.ay, C.span, C.ids.as<int32_t>(), C.cfirst.as<int64_t>(), C.cu.as<uint64_t>(),
                          C.cboff.as<int64_t>(), C.d_qc.as<int64_t>(), C.d_qb.as<int64_t>(), B.mp_off.as<int64_t>(), B.d_qlen.as<int64_t>(), B.d_hash, B.rep_len.as<int32_t>(), B.idx->d_len,
                          B.n_q, B.opt, B.idx->k, z.p, rg.as<hymet_mm_reg>(), wv.as<int32_t>(), cov.as<uint64_t>(),
                          tmp.as<int32_t>(), nr.as<int32_t>(), C.n_anchor, NC, C.cq.as<uint32_t>(),
                          B.pos_tab.as<MiniWord>(), B.d_qbase.as<int64_t>(), skip_q);
}

// one chain set's region records: where reg_gather_kernel reads a query's regions from
struct RegSet {
    const int32_t *n;      // per query: regions
    const int64_t *qc;     // per query: offset of its first record
    const hymet_mm_reg *r;
};

// PAF order within the batch: query by query, each query's regions as selected -- those of
// set 2 for the queries flagged in fl (nullable), of set 1 for the others -- into the sink
static int emit_records(MapBatch &B, const uint32_t *fl, const RegSet &s1, const RegSet &s2, MapSink &sink) {
    hymet_ctx *ctx = B.ctx;
    hipStream_t st = ctx->stream;
    const int n_q = B.n_q;
    hymet_mm_result *res = sink.res;
    DevBuf cnt, off;
    HY_HIP(cnt.alloc(4 * (size_t)(n_q + 1), st));
    LAUNCH1(reg_count_kernel, n_q, fl, s1.n, s2.n, n_q, cnt.as<uint32_t>());
    int64_t N = 0;
    int rc = scan_flags(ctx, cnt.as<uint32_t>(), n_q, off, &N);
    if (rc) return rc;
    HY_HIP(hipMemcpyAsync(off.as<int64_t>() + n_q, &N, 8, hipMemcpyHostToDevice, st));
    RegOut o{};
    DevBuf tmp_regs;
    if (sink.acc) {
        hymet_paf_acc *a = sink.acc;
        rc = acc_reserve(ctx, a, a->n + N);
        if (rc) return rc;
        o = RegOut{a->regs.as<hymet_mm_reg>() + a->n, a->q.as<int32_t>() + a->n, a->part.as<int32_t>() + a->n,
                   a->rl.as<int32_t>() + a->n, a->t.as<int32_t>() + a->n, sink.q_base, sink.part_id, sink.t_base};
    } else {
        HY_HIP(tmp_regs.alloc(sizeof(hymet_mm_reg) * (size_t)(N + 1), st));
        o.regs = tmp_regs.as<hymet_mm_reg>();
    }
    {
        ProfScope _ps(ctx, "mm_paf_records", (double)N * (2.0 * sizeof(hymet_mm_reg) + 16.0));
        LAUNCH1(reg_gather_kernel, n_q, fl, s1.n, s2.n, s1.qc, s2.qc, s1.r, s2.r, off.as<int64_t>(), B.rep_len.as<int32_t>(),
                n_q, o);
    }
    if (sink.acc) {
        sink.acc->n += N;
    } else {
        res->regs.resize(N);
        if (N) HY_HIP(hipMemcpyAsync(res->regs.data(), tmp_regs.p, sizeof(hymet_mm_reg) * (size_t)N, hipMemcpyDeviceToHost, st));
        HY_HIP(hipMemcpyAsync(res->reg_off.data(), off.p, 8 * (size_t)(n_q + 1), hipMemcpyDeviceToHost, st));
        HY_HIP(hipMemcpyAsync(res->rep_len.data(), B.rep_len.p, 4 * (size_t)n_q, hipMemcpyDeviceToHost, st));
    }
    // host vectors above are async copy sources/targets
    HY_HIP(hipStreamSynchronize(st));
    return HYMET_OK;
}

static int mm_map_impl(hymet_ctx *ctx, const hymet_mm_index *idx, const hymet_mm_opt *opt, const uint32_t *d_2b,
                       const uint32_t *d_mask, const int64_t *h_starts, const int64_t *h_lens, const uint32_t *h_name_hash,
                       const uint32_t *d_name_hash, int32_t n_q, MapSink &sink) {
    CallTrace call_trace;
    HY_ARG(ctx && idx && opt && d_2b && d_mask, "hymet_mm_map: null argument");
    HY_ARG(n_q >= 0, "hymet_mm_map: n_q < 0");
    HY_ARG(h_name_hash || d_name_hash, "hymet_mm_map: no query name hashes");
    HY_ARG(opt->mid_occ > 0, "hymet_mm_map: opt->mid_occ must be resolved (hymet_mm_index_max_occ + clamps)");
    HY_HIP(hipSetDevice(ctx->device));
    if (sink.res) {
        sink.res->n_q = n_q;
        sink.res->reg_off.assign(n_q + 1, 0);
        sink.res->rep_len.assign(n_q, 0);
    }
    if (n_q == 0) return HYMET_OK;
    const float pen_gap = (float)(opt->chain_gap_scale * 0.01 * idx->k);
    const float pen_skip = (float)(opt->chain_skip_scale * 0.01 * idx->k);
    PhaseTrace tr(ctx);
    MapBatch B{ctx, idx, opt, h_lens, n_q};
    int rc = sketch_queries(B, d_2b, d_mask, h_starts, h_name_hash, d_name_hash);
    if (rc) return rc;
    tr.mark("sketch");
    rc = filter_minimizers(B);
    if (rc) return rc;
    tr.mark("mz_flt");
    rc = select_seeds(B);
    if (rc) return rc;
    tr.mark("seeds");
    AnchorSet S1;
    rc = first_pass_anchors(B, S1);
    if (rc) return rc;
    tr.mark("anchors+sort");
    static std::atomic<bool> dumped1{false};
    rc = dump_anchors(ctx, "HYMET_DUMP_ANCHORS", S1, n_q, dumped1);
    if (rc) return rc;
    // ------------------------------------------------ 6 chain (+ 7 long join)
    ChainSet C1;
    const bool long_join = opt->bw_long > opt->bw;
    LeanJoin lj{B.d_qlen.as<int64_t>(), opt->rmq_rescue_size, opt->rmq_rescue_ratio};
    rc = chain_set(ctx, opt, pen_gap, pen_skip, opt->bw, S1, n_q, C1, long_join ? &lj : nullptr);
    if (rc) return rc;
    tr.mark("chain_set 1");
    ChainSet C2;
    AnchorSet S2;  // the long join's anchors: its chains (C2) are read in place until the regions
    DevBuf flag;   // queries re-chained by the long join (their first-pass regions are not built)
    bool joined = false;
    if (long_join && C1.n_chain > 0) {
        flag.swap(lj.flag);
        rc = long_join_anchors(B, S1, lj, flag, S2, joined);
        if (rc) return rc;
        if (joined) {  // flagged queries take C2's chains, the others keep C1's
            rc = chain_set(ctx, opt, pen_gap, pen_skip, opt->bw_long, S2, n_q, C2);
            if (rc) return rc;
        }
    }
    tr.mark("long join");
    // -------------------------------------------------------------- 8 regions
    // region records stay in HBM: per chain set, records at the set's chain offsets + counts
    DevBuf rg1, nr1, rg2, nr2;
    const uint32_t *fl = joined ? flag.as<uint32_t>() : nullptr;
    rc = run_regions(B, C1, rg1, nr1, fl);
    if (rc) return rc;
    if (joined) {
        rc = run_regions(B, C2, rg2, nr2, nullptr);
        if (rc) return rc;
    }
    const RegSet r1{nr1.as<int32_t>(), C1.d_qc.as<int64_t>(), rg1.as<hymet_mm_reg>()};
    const RegSet r2{nr2.as<int32_t>(), C2.d_qc.as<int64_t>(), rg2.as<hymet_mm_reg>()};
    rc = emit_records(B, fl, r1, joined ? r2 : r1, sink);
    if (rc) return rc;
    tr.mark("regions");
    return HYMET_OK;
}

extern "C" {

int hymet_mm_map(hymet_ctx *ctx, const hymet_mm_index *idx, const hymet_mm_opt *opt, const uint32_t *d_2b,
                 const uint32_t *d_mask, const int64_t *h_starts, const int64_t *h_lens, const uint32_t *h_name_hash,
                 int32_t n_q, hymet_mm_result **out) {
    HY_ARG(out != nullptr, "hymet_mm_map: null argument");
    MapSink sink;
    sink.res = new hymet_mm_result();
    *out = sink.res;
    return mm_map_impl(ctx, idx, opt, d_2b, d_mask, h_starts, h_lens, h_name_hash, nullptr, n_q, sink);
}

int hymet_paf_acc_create(hymet_ctx *ctx, hymet_paf_acc **out) {
    HY_ARG(ctx && out, "hymet_paf_acc_create: null argument");
    hymet_paf_acc *a = new hymet_paf_acc();
    a->device = ctx->device;
    *out = a;
    return HYMET_OK;
}

int hymet_paf_acc_reset(hymet_paf_acc *acc) {
    HY_ARG(acc, "hymet_paf_acc_reset: null argument");
    acc->n = 0;
    return HYMET_OK;
}

int hymet_paf_acc_destroy(hymet_paf_acc *acc) {
    if (acc) {
        (void)hipSetDevice(acc->device);
        delete acc;
    }
    return HYMET_OK;
}

int hymet_paf_acc_info(const hymet_paf_acc *acc, int64_t *n_lines, void **d_regs, void **d_q, void **d_part, void **d_rl,
                       void **d_t) {
    HY_ARG(acc && n_lines, "hymet_paf_acc_info: null argument");
    *n_lines = acc->n;
    if (d_regs) *d_regs = acc->regs.p;
    if (d_q) *d_q = acc->q.p;
    if (d_part) *d_part = acc->part.p;
    if (d_rl) *d_rl = acc->rl.p;
    if (d_t) *d_t = acc->t.p;
    return HYMET_OK;
}

int hymet_paf_acc_append(hymet_ctx *ctx, hymet_paf_acc *dst, const hymet_paf_acc *src, int64_t begin, int64_t end) {
    HY_ARG(ctx && dst && src && dst != src, "hymet_paf_acc_append: null or aliased argument");
    HY_ARG(begin >= 0 && end >= begin && end <= src->n, "hymet_paf_acc_append: line range outside the source");
    const int64_t m = end - begin;
    if (m == 0) return HYMET_OK;
    HY_HIP(hipSetDevice(ctx->device));
    int rc = acc_reserve(ctx, dst, dst->n + m);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const int64_t d = dst->n;
    HY_HIP(hipMemcpyAsync(dst->regs.as<hymet_mm_reg>() + d, src->regs.as<hymet_mm_reg>() + begin, sizeof(hymet_mm_reg) * (size_t)m,
                          hipMemcpyDeviceToDevice, st));
    HY_HIP(hipMemcpyAsync(dst->q.as<int32_t>() + d, src->q.as<int32_t>() + begin, 4 * (size_t)m, hipMemcpyDeviceToDevice, st));
    HY_HIP(hipMemcpyAsync(dst->part.as<int32_t>() + d, src->part.as<int32_t>() + begin, 4 * (size_t)m, hipMemcpyDeviceToDevice,
                          st));
    HY_HIP(hipMemcpyAsync(dst->rl.as<int32_t>() + d, src->rl.as<int32_t>() + begin, 4 * (size_t)m, hipMemcpyDeviceToDevice, st));
    HY_HIP(hipMemcpyAsync(dst->t.as<int32_t>() + d, src->t.as<int32_t>() + begin, 4 * (size_t)m, hipMemcpyDeviceToDevice, st));
    dst->n += m;
    return HYMET_OK;
}

int hymet_paf_acc_copy(hymet_ctx *ctx, const hymet_paf_acc *acc, int32_t *h_q, int32_t *h_part, int32_t *h_t) {
    HY_ARG(ctx && acc, "hymet_paf_acc_copy: null argument");
    if (acc->n <= 0) return HYMET_OK;
    HY_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (h_q) HY_HIP(hipMemcpyAsync(h_q, acc->q.p, 4 * (size_t)acc->n, hipMemcpyDeviceToHost, st));
    if (h_part) HY_HIP(hipMemcpyAsync(h_part, acc->part.p, 4 * (size_t)acc->n, hipMemcpyDeviceToHost, st));
    if (h_t) HY_HIP(hipMemcpyAsync(h_t, acc->t.p, 4 * (size_t)acc->n, hipMemcpyDeviceToHost, st));
    HY_HIP(hipStreamSynchronize(st));
    return HYMET_OK;
}

int hymet_paf_acc_field(hymet_ctx *ctx, const hymet_paf_acc *acc, int field, int32_t *h_out) {
    HY_ARG(ctx && acc && h_out && field >= 0 && field < (int)(sizeof(hymet_mm_reg) / 4), "hymet_paf_acc_field: bad argument");
    if (acc->n <= 0) return HYMET_OK;
    HY_HIP(hipSetDevice(ctx->device));
    const char *src = static_cast<const char *>(acc->regs.p) + 4 * (size_t)field;
    HY_HIP(hipMemcpy2DAsync(h_out, 4, src, sizeof(hymet_mm_reg), 4, (size_t)acc->n, hipMemcpyDeviceToHost, ctx->stream));
    HY_HIP(hipStreamSynchronize(ctx->stream));
    return HYMET_OK;
}

int hymet_mm_map_acc(hymet_ctx *ctx, const hymet_mm_index *idx, const hymet_mm_opt *opt, const uint32_t *d_2b,
                     const uint32_t *d_mask, const int64_t *h_starts, const int64_t *h_lens, const uint32_t *d_name_hash,
                     int32_t n_q, int32_t q_base, int32_t part_id, int32_t t_base, hymet_paf_acc *acc) {
    HY_ARG(acc && d_name_hash, "hymet_mm_map_acc: null argument");
    MapSink sink;
    sink.acc = acc;
    sink.q_base = q_base;
    sink.part_id = part_id;
    sink.t_base = t_base;
    return mm_map_impl(ctx, idx, opt, d_2b, d_mask, h_starts, h_lens, nullptr, d_name_hash, n_q, sink);
}

int hymet_mm_result_size(const hymet_mm_result *res, int64_t *n_regs) {
    HY_ARG(res && n_regs, "hymet_mm_result_size: null argument");
    *n_regs = (int64_t)res->regs.size();
    return HYMET_OK;
}

int hymet_mm_result_copy(const hymet_mm_result *res, int64_t *h_off, int32_t *h_rep_len, hymet_mm_reg *h_regs) {
    HY_ARG(res, "hymet_mm_result_copy: null result");
    if (h_off) memcpy(h_off, res->reg_off.data(), 8 * (size_t)(res->n_q + 1));
    if (h_rep_len && res->n_q) memcpy(h_rep_len, res->rep_len.data(), 4 * (size_t)res->n_q);
    if (h_regs && !res->regs.empty()) memcpy(h_regs, res->regs.data(), sizeof(hymet_mm_reg) * res->regs.size());
    return HYMET_OK;
}

int hymet_mm_result_destroy(hymet_mm_result *res) {
    delete res;
    return HYMET_OK;
}

}  // extern "C"

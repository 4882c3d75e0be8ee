// Per-probe top-k for k up to 1024 (the shortlist of a 1:N identification): the ranking of
// rank.hip (by the ranking key of rank_key.h, unique per element: descending, ties to the lower
// index, NaN after every number) without k passes over the row.
//
//   1. Radix search for the k-th largest key T: six digit passes over the key's 64 bits from the top
//      (five of 11 bits, one of 9).  A pass is one launch of several workgroups per row; each builds
//      the histogram of its slice's keys that match the prefix found so far (LDS, then integer
//      atomics into the row's global histogram: the counts do not depend on arrival order).  The
//      prefix of pass d is derived at the start of pass d from pass d - 1's finished histogram, by
//      every workgroup for itself; workgroup 0 of the row records it for pass d + 1.  Launch order on
//      the stream is the only synchronisation.
//   2. Compaction: the keys >= T (exactly k, keys being unique) go to a k-slot list, slots handed
//      out by an integer atomic (their order is arbitrary and does not matter:)
//   3. one workgroup per row sorts the list in LDS (bitonic, 1024 slots) and writes indices and scores.
//
// fpm_rank_keep (the prescreen of a 1:N identification) takes step 1 as it is (rs_search) for any k <= G and
// replaces steps 2 and 3 by an ordered compaction: the columns whose key is >= T, in ascending column order,
// with no slot handed out by an atomic (below).
#include "rank_key.h"
#include "fpm.h"

namespace {
using namespace fpm;
constexpr int RS_THREADS = 256;
constexpr int RS_KMAX = FPM_RANK_SELECT_KMAX;
constexpr int RS_PASSES = 6;
constexpr int RS_BINS = 2048;
constexpr int RS_ITEMS = 16;                       // elements per thread and slice pass

__device__ __host__ constexpr int rs_width(int d) { return d < 5 ? 11 : 9; }
__device__ __host__ constexpr int rs_shift(int d) { return d < 5 ? 53 - 11 * d : 0; }

// per-row scratch
struct RsRow {
    unsigned hist[RS_PASSES][RS_BINS];
    u64 prefix[RS_PASSES + 1];     // prefix[d]: the key bits above pass d's digit; prefix[6] = T
    unsigned krem[RS_PASSES + 1];  // rank still sought among the keys that match prefix[d]
    unsigned count;                // compaction slots handed out
    unsigned pad;
    u64 cand[RS_KMAX];
};

// prefix / remaining rank of pass d (1 <= d <= 6) from pass d - 1's state and finished histogram;
// every thread of the workgroup returns with the same pair.  sh: RS_THREADS + 2 words of LDS.
__device__ void rs_derive(const RsRow* w, int d, unsigned k, unsigned* sh, u64& prefix, unsigned& krem) {
    if (d == 0) {
        prefix = 0;
        krem = k;
        return;
    }
    const u64 pp = d == 1 ? 0ull : w->prefix[d - 1];
    const unsigned kr = d == 1 ? k : w->krem[d - 1];
    const unsigned* h = w->hist[d - 1];
    const int tid = threadIdx.x;
    // thread t owns the 8 bins 2047 - 8t .. 2040 - 8t (descending walk)
    unsigned c[8], ls = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        c[q] = h[RS_BINS - 1 - (8 * tid + q)];
        ls += c[q];
    }
    sh[tid] = ls;
    __syncthreads();
    for (int o = 1; o < RS_THREADS; o <<= 1) {       // inclusive scan over the threads
        const unsigned v = tid >= o ? sh[tid - o] : 0u;
        __syncthreads();
        sh[tid] += v;
        __syncthreads();
    }
    unsigned above = sh[tid] - ls;                   // keys in bins above this thread's
    if (above < kr && kr <= above + ls) {            // exactly one thread: the bin of rank kr
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (above < kr && kr <= above + c[q]) {
                sh[RS_THREADS] = (unsigned)(RS_BINS - 1 - (8 * tid + q));
                sh[RS_THREADS + 1] = kr - above;
            }
            above += c[q];
        }
    }
    __syncthreads();
    prefix = (pp << rs_width(d - 1)) | sh[RS_THREADS];
    krem = sh[RS_THREADS + 1];
    __syncthreads();
}

__global__ __launch_bounds__(RS_THREADS) void rank_select_hist_kernel(const float* __restrict__ scores, long ld, int G,
                                                                      int k, int d, RsRow* __restrict__ ws) {
    __shared__ unsigned lh[RS_BINS];
    __shared__ unsigned sh[RS_THREADS + 2];
    RsRow* w = ws + blockIdx.y;
    const float* row = scores + (long)blockIdx.y * ld;
    u64 prefix;
    unsigned krem;
    rs_derive(w, d, (unsigned)k, sh, prefix, krem);
    if (blockIdx.x == 0 && threadIdx.x == 0 && d > 0) {
        w->prefix[d] = prefix;
        w->krem[d] = krem;
    }
    for (int i = threadIdx.x; i < RS_BINS; i += RS_THREADS) lh[i] = 0u;
    __syncthreads();
    const int sh_d = rs_shift(d), wd = rs_width(d);
    const long per = (long)RS_THREADS * RS_ITEMS;
    for (long base = (long)blockIdx.x * per; base < G; base += (long)gridDim.x * per) {
#pragma unroll 4
        for (int q = 0; q < RS_ITEMS; ++q) {
            const long i = base + q * RS_THREADS + threadIdx.x;
            if (i < G) {
                const u64 key = rank_key(row[i], (uint32_t)i);
                if (d == 0 || (key >> (sh_d + wd)) == prefix)
                    atomicAdd(&lh[(unsigned)(key >> sh_d) & ((1u << wd) - 1u)], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < RS_BINS; i += RS_THREADS)
        if (lh[i]) atomicAdd(&w->hist[d][i], lh[i]);
}

__global__ __launch_bounds__(RS_THREADS) void rank_select_compact_kernel(const float* __restrict__ scores, long ld,
                                                                         int G, int k, RsRow* __restrict__ ws) {
    __shared__ unsigned sh[RS_THREADS + 2];
    RsRow* w = ws + blockIdx.y;
    const float* row = scores + (long)blockIdx.y * ld;
    u64 T;
    unsigned krem;
    rs_derive(w, RS_PASSES, (unsigned)k, sh, T, krem);
    const long per = (long)RS_THREADS * RS_ITEMS;
    for (long base = (long)blockIdx.x * per; base < G; base += (long)gridDim.x * per) {
        for (int q = 0; q < RS_ITEMS; ++q) {
            const long i = base + q * RS_THREADS + threadIdx.x;
            if (i < G) {
                const u64 key = rank_key(row[i], (uint32_t)i);
                if (key >= T) {
                    const unsigned slot = atomicAdd(&w->count, 1u);
                    if (slot < (unsigned)k) w->cand[slot] = key;     // exactly k keys pass; the guard bounds the write
                }
            }
        }
    }
}

__global__ __launch_bounds__(RS_THREADS) void rank_select_sort_kernel(const float* __restrict__ scores, long ld, int G, int k,
                                                                      const RsRow* __restrict__ ws,
                                                                      int* __restrict__ top_idx,
                                                                      float* __restrict__ top_score) {
    __shared__ u64 key[RS_KMAX];
    const RsRow* w = ws + blockIdx.x;
    const float* row = scores + (long)blockIdx.x * ld;
    int n = 2;
    while (n < k) n <<= 1;                           // power of two >= k, at most 1024
    for (int i = threadIdx.x; i < n; i += RS_THREADS) key[i] = i < k ? w->cand[i] : 0ull;   // 0 is below every key
    __syncthreads();
    for (int size = 2; size <= n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < n / 2; t += RS_THREADS) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const u64 a = key[lo], b = key[hi];
                if ((a < b) == desc) {
                    key[lo] = b;
                    key[hi] = a;
                }
            }
            __syncthreads();
        }
    for (int j = threadIdx.x; j < k; j += RS_THREADS) {
        const uint32_t i = rank_index(key[j]);
        const bool ok = i < (uint32_t)G;             // always, with k <= G keys in the list; never read outside the row
        top_idx[(long)blockIdx.x * k + j] = ok ? (int)i : -1;
        top_score[(long)blockIdx.x * k + j] = ok ? row[i] : qnan();
    }
}

// ---- rank_keep: the k best of a row as a set, in column order, for any k <= G ------------------------------
// The row is cut into contiguous slices of RK_CHUNK-aligned length; slice s of row p is one workgroup in both
// launches.  Launch 1: the slice's count of keys >= T.  Launch 2: the sum of the counts of the slices before it
// (fixed order), then the slice's columns in ascending order, a chunk of 256 at a time: the place inside a chunk
// is the wave's ballot prefix plus the counts of the waves before it.
constexpr int RK_CHUNK = RS_THREADS;
constexpr int RK_SLICE = RS_THREADS * RS_ITEMS;     // columns per slice, at least
constexpr int RK_SLICES = 1024;                     // slices per row, at most

struct RkPlan {
    int nb;        // slices per row
    long len;      // columns per slice (a multiple of RK_CHUNK)
};
inline RkPlan rk_plan(int G) {
    long nb = ((long)G + RK_SLICE - 1) / RK_SLICE;
    nb = nb < 1 ? 1 : (nb > RK_SLICES ? RK_SLICES : nb);
    long len = ((long)G + nb - 1) / nb;
    len = (len + RK_CHUNK - 1) / RK_CHUNK * RK_CHUNK;
    nb = ((long)G + len - 1) / len;
    return RkPlan{(int)(nb < 1 ? 1 : nb), len};
}

// the sum of v over the workgroup, in every thread (a fixed tree over LDS; sh: RS_THREADS words)
__device__ unsigned rk_block_sum(unsigned v, unsigned* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int o = RS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    const unsigned r = sh[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(RS_THREADS) void rank_keep_count_kernel(const float* __restrict__ scores, long ld, int G,
                                                                     int k, long len, const RsRow* __restrict__ ws,
                                                                     unsigned* __restrict__ cnt) {
    __shared__ unsigned sh[RS_THREADS + 2];
    const RsRow* w = ws + blockIdx.y;
    const float* row = scores + (long)blockIdx.y * ld;
    u64 T;
    unsigned krem;
    rs_derive(w, RS_PASSES, (unsigned)k, sh, T, krem);
    const long c0 = (long)blockIdx.x * len, c1 = c0 + len < G ? c0 + len : G;
    unsigned c = 0;
    for (long i = c0 + threadIdx.x; i < c1; i += RS_THREADS) c += rank_key(row[i], (uint32_t)i) >= T ? 1u : 0u;
    c = rk_block_sum(c, sh);
    if (threadIdx.x == 0) cnt[(long)blockIdx.y * gridDim.x + blockIdx.x] = c;
}

__global__ __launch_bounds__(RS_THREADS) void rank_keep_write_kernel(const float* __restrict__ scores, long ld, int G,
                                                                     int k, long len, const RsRow* __restrict__ ws,
                                                                     const unsigned* __restrict__ cnt,
                                                                     int* __restrict__ keep) {
    __shared__ unsigned sh[RS_THREADS + 2];
    __shared__ unsigned wc[RS_THREADS / 64];
    const RsRow* w = ws + blockIdx.y;
    const float* row = scores + (long)blockIdx.y * ld;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    u64 T;
    unsigned krem;
    rs_derive(w, RS_PASSES, (unsigned)k, sh, T, krem);
    // columns kept by the slices before this one
    unsigned before = 0;
    for (int s = tid; s < (int)blockIdx.x; s += RS_THREADS) before += cnt[(long)blockIdx.y * gridDim.x + s];
    unsigned base = rk_block_sum(before, sh);
    int* out = keep + (long)blockIdx.y * k;
    const long c0 = (long)blockIdx.x * len, c1 = c0 + len < G ? c0 + len : G;
    for (long b = c0; b < c1; b += RK_CHUNK) {               // the trip count is the workgroup's
        const long i = b + tid;
        const bool in = i < c1 && rank_key(row[i < c1 ? i : c0], (uint32_t)i) >= T;
        const u64 m = __ballot(in);
        if (lane == 0) wc[wv] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned at = base, all = 0;
#pragma unroll
        for (int q = 0; q < RS_THREADS / 64; ++q) {
            if (q < wv) at += wc[q];
            all += wc[q];
        }
        at += (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (in && at < (unsigned)k) out[at] = (int)i;        // exactly k columns pass; the guard bounds the write
        base += all;
        __syncthreads();
    }
}

// the grid of the search's passes and of rank_select's compaction: several workgroups per row
inline dim3 rs_grid(int P, int G) {
    const long per = (long)RS_THREADS * RS_ITEMS;
    long nb = (G + per - 1) / per;
    nb = nb < 1 ? 1 : (nb > 256 ? 256 : nb);
    return dim3((unsigned)nb, (unsigned)P);
}

// step 1 of both entry points: the six digit passes over a cleared workspace
void rs_search(const float* scores, long ld, int P, int G, int k, RsRow* w, hipStream_t st) {
    for (int d = 0; d < RS_PASSES; ++d)
        hipLaunchKernelGGL(rank_select_hist_kernel, rs_grid(P, G), dim3(RS_THREADS), 0, st, scores, ld, G, k, d, w);
}
}  // namespace

extern "C" long fpm_rank_select_ws_bytes(int P) { return P > 0 ? (long)P * (long)sizeof(RsRow) : 0; }

extern "C" int fpm_rank_select(const float* scores, long ld, int P, int G, int k, int* top_idx, float* top_score,
                               void* ws, long ws_bytes, void* stream) {
    FPM_CHECK_ARG(P >= 0 && G >= 1 && ld >= G, "rank_select: bad sizes (P %d, G %d, ld %ld)", P, G, ld);
    FPM_CHECK_ARG(k >= 1 && k <= RS_KMAX && k <= G, "rank_select: k = %d outside [1, min(G, %d)]", k, RS_KMAX);
    FPM_CHECK_ARG(scores && top_idx && top_score, "rank_select: scores, top_idx and top_score are required");
    FPM_CHECK_ARG(P <= 65535, "rank_select: at most 65535 rows per call (P %d)", P);
    if (P == 0) return 0;
    const long need = fpm_rank_select_ws_bytes(P);
    FPM_CHECK_ARG(ws && ws_bytes >= need, "rank_select: workspace of %ld bytes required (got %ld)", need, ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, (size_t)need, st) != hipSuccess) {
        (void)hipGetLastError();
        fpm::set_error("rank_select: clearing the workspace failed");
        return 1;
    }
    RsRow* w = (RsRow*)ws;
    rs_search(scores, ld, P, G, k, w, st);
    hipLaunchKernelGGL(rank_select_compact_kernel, rs_grid(P, G), dim3(RS_THREADS), 0, st, scores, ld, G, k, w);
    hipLaunchKernelGGL(rank_select_sort_kernel, dim3((unsigned)P), dim3(RS_THREADS), 0, st, scores, ld, G, k,
                       (const RsRow*)w, top_idx, top_score);
    return fpm::check_launch("fpm_rank_select");
}

extern "C" long fpm_rank_keep_ws_bytes(int P, int G) {
    if (P <= 0 || G <= 0) return 0;
    return (long)P * ((long)sizeof(RsRow) + (long)rk_plan(G).nb * (long)sizeof(unsigned));
}

extern "C" int fpm_rank_keep(const float* scores, long ld, int P, int G, int k, int* keep, void* ws, long ws_bytes,
                             void* stream) {
    FPM_CHECK_ARG(P >= 0 && G >= 1 && ld >= G, "rank_keep: bad sizes (P %d, G %d, ld %ld)", P, G, ld);
    FPM_CHECK_ARG(k >= 1 && k <= G, "rank_keep: k = %d outside [1, G = %d]", k, G);
    FPM_CHECK_ARG(scores && keep, "rank_keep: scores and keep are required");
    FPM_CHECK_ARG(P <= 65535, "rank_keep: at most 65535 rows per call (P %d)", P);
    if (P == 0) return 0;
    const long need = fpm_rank_keep_ws_bytes(P, G);
    FPM_CHECK_ARG(ws && ws_bytes >= need, "rank_keep: workspace of %ld bytes required (got %ld)", need, ws_bytes);
    FPM_CHECK_ARG(((uintptr_t)ws & 7) == 0, "rank_keep: the workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, (size_t)need, st) != hipSuccess) {
        (void)hipGetLastError();
        fpm::set_error("rank_keep: clearing the workspace failed");
        return 1;
    }
    RsRow* w = (RsRow*)ws;
    unsigned* cnt = (unsigned*)(w + P);
    const RkPlan pl = rk_plan(G);
    rs_search(scores, ld, P, G, k, w, st);
    const dim3 grid((unsigned)pl.nb, (unsigned)P);
    hipLaunchKernelGGL(rank_keep_count_kernel, grid, dim3(RS_THREADS), 0, st, scores, ld, G, k, pl.len,
                       (const RsRow*)w, cnt);
    hipLaunchKernelGGL(rank_keep_write_kernel, grid, dim3(RS_THREADS), 0, st, scores, ld, G, k, pl.len,
                       (const RsRow*)w, (const unsigned*)cnt, keep);
    return fpm::check_launch("fpm_rank_keep");
}

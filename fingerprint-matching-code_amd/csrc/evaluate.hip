// Evaluation of a 1:N search from its score matrices: the rank of every probe's mate, the census of genuine
// and impostor scores over a grid of edges, and the k-th largest score of a class (a FAR threshold).  All
// three read a (P, G) fp32 matrix once or twice at memory bandwidth and are integer-exact: maxima of 64-bit
// keys and integer sums, which do not depend on the order of arrival.  No float atomics.
//
// Classes of a score (p, j): ignored when col_lab < 0 or j == own[p]; genuine when col_lab == row_lab[p];
// impostor otherwise.  col_lab is read at col_lab + p * lab_ld (lab_ld 0: one row of labels for all probes).
// Ordering: the ranking key of rank_key.h over (score, column): score descending, ties to the lower column,
// NaN after every number, -0 below +0.
//
// Grid (slices of EV_SLICE columns, rows): 256 threads, thread t of slice s holds the columns
// s * 4096 + t + 256 i, i < 16 (coalesced, 16 loads in flight), and walks the rows blockIdx.y, + gridDim.y, ...
// With shared labels a thread's 16 labels are loaded once for all its rows.
//
//   mate_max    per (slice, row): the largest genuine key -> one 64-bit atomic max on best[row]
//   mate_count  per (slice, row): impostor keys above best[row] -> one 32-bit integer add on rank[row];
//               slice 0 writes the mate's column and score bits (and -1 / NaN / -1 for a row without a mate)
//   tally<0>    census: 32-bit LDS histograms of the workgroup's rows (bin = number of edges <= score, a
//               binary search of fixed length over the edges in LDS, a thread's 16 searches step by step
//               together; the edges padded with NaN to a power of two less one, so a step is an add, a read, a
//               compare and a select), one 64-bit atomic add per non-empty bin; LDS by T, at most 48 KB
//   tally<1>    radix pass: the same over a digit of the score bits, for the scores of one class that match the
//               prefix found so far; three passes (11, 11, 10 bits), the histogram read on the host in between
#include "rank_key.h"
#include "fpm.h"

namespace {
using namespace fpm;
constexpr int EV_THREADS = 256;
constexpr int EV_PER = 16;
constexpr int EV_SLICE = EV_THREADS * EV_PER;      // 4096 columns per workgroup
constexpr int EV_TMAX = 4095;                      // edges of a census
constexpr int EV_ROWS_MAX = 1 << 19;               // rows per workgroup: 2^19 * 4096 = 2^31 fits an LDS counter
constexpr int EV_TALLY_BLOCKS = 1024;              // workgroups of a tally launch (about four per CU)
constexpr int EV_RADIX_BINS = 2048;

struct EvalIn {
    const float* scores;
    long ld;
    int P, G;
    const int* row_lab;
    const int* col_lab;
    long lab_ld;
    const int* own;                                // or null
};

// The rows of this workgroup, its slice of each: begin(p), elem(p, i, j, x, cls) for the thread's i-th column j, if j < G
// (cls 0 ignored, 1 genuine, 2 impostor), end(p).  The trip counts are uniform over the workgroup.
template <typename Begin, typename Elem, typename End>
__device__ __forceinline__ void ev_walk(const EvalIn& in, Begin&& begin, Elem&& elem, End&& end) {
    const long j0 = (long)blockIdx.x * EV_SLICE + threadIdx.x;
    int cl[EV_PER];
    if (in.lab_ld == 0) {
#pragma unroll
        for (int i = 0; i < EV_PER; ++i) {
            const long j = j0 + i * EV_THREADS;
            cl[i] = j < in.G ? in.col_lab[j] : -1;
        }
    }
    for (long p = blockIdx.y; p < in.P; p += gridDim.y) {
        const float* row = in.scores + p * in.ld;
        if (in.lab_ld != 0) {
            const int* lab = in.col_lab + p * in.lab_ld;
#pragma unroll
            for (int i = 0; i < EV_PER; ++i) {
                const long j = j0 + i * EV_THREADS;
                cl[i] = j < in.G ? lab[j] : -1;
            }
        }
        float x[EV_PER];
#pragma unroll
        for (int i = 0; i < EV_PER; ++i) {
            const long j = j0 + i * EV_THREADS;
            x[i] = j < in.G ? row[j] : 0.f;
        }
        const int rl = in.row_lab[p];
        const int ow = in.own ? in.own[p] : -1;
        begin(p);
#pragma unroll
        for (int i = 0; i < EV_PER; ++i) {
            const long j = j0 + i * EV_THREADS;
            if (j < in.G) {
                const int c = (cl[i] < 0 || (int)j == ow) ? 0 : (cl[i] == rl ? 1 : 2);
                elem(p, i, (int)j, x[i], c);
            }
        }
        end(p);
    }
}

__global__ __launch_bounds__(EV_THREADS) void mate_max_kernel(EvalIn in, u64* __restrict__ best) {
    __shared__ u64 part[EV_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 b = 0ull;                                  // below every key
    ev_walk(
        in, [&](long) { b = 0ull; },
        [&](long, int, int j, float x, int c) {
            const u64 key = rank_key(x, (uint32_t)j);
            if (c == 1 && key > b) b = key;
        },
        [&](long p) {
            b = team_max_u64<64>(b);
            if (lane == 0) part[wave] = b;
            __syncthreads();
            if (threadIdx.x == 0) {
                u64 m = part[0];
#pragma unroll
                for (int w = 1; w < EV_THREADS / 64; ++w) m = part[w] > m ? part[w] : m;
                if (m) atomicMax(best + p, m);
            }
            __syncthreads();
        });
}

__global__ __launch_bounds__(EV_THREADS) void mate_count_kernel(EvalIn in, const u64* __restrict__ best,
                                                                int* __restrict__ mate_col,
                                                                float* __restrict__ mate_score,
                                                                int* __restrict__ mate_rank) {
    __shared__ int part[EV_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 T = 0ull;
    int cnt = 0;
    ev_walk(
        in,
        [&](long p) {
            T = best[p];
            cnt = 0;
        },
        [&](long, int, int j, float x, int c) { cnt += (c == 2 && T != 0ull && rank_key(x, (uint32_t)j) > T) ? 1 : 0; },
        [&](long p) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
            if (lane == 0) part[wave] = cnt;
            __syncthreads();
            if (threadIdx.x == 0) {
                int tot = 0;
#pragma unroll
                for (int w = 0; w < EV_THREADS / 64; ++w) tot += part[w];
                if (tot) atomicAdd(mate_rank + p, tot);            // rank[p] was cleared before the launch
                if (blockIdx.x == 0) {
                    if (T == 0ull) {                                // no mate: no workgroup adds to this row
                        mate_col[p] = -1;
                        mate_score[p] = qnan();
                        mate_rank[p] = -1;
                    } else {
                        const int col = (int)rank_index(T);
                        mate_col[p] = col;
                        mate_score[p] = in.scores[p * in.ld + col];
                    }
                }
            }
            __syncthreads();
        });
}

struct TallyArgs {
    const float* edges;                            // MODE 0
    int T, top;                                    // top: the largest power of two <= T
    int want, shift, width, hi_shift;              // MODE 1: the class, the digit, where the prefix starts
    uint32_t prefix;
    u64* out_a;                                    // MODE 0: gen (T + 1); MODE 1: the digit's histogram
    u64* out_b;                                    // MODE 0: imp (T + 1)
    u64* skipped;                                  // MODE 0: NaN genuine, NaN impostor, ignored
};

template <int MODE>
__global__ __launch_bounds__(EV_THREADS) void tally_kernel(EvalIn in, TallyArgs a) {
    extern __shared__ uint32_t ev_lds[];           // MODE 0: gen and imp bins, then the T edges; MODE 1: the digit's bins
    __shared__ uint32_t skip[3];
    const int nb = MODE == 0 ? 2 * (a.T + 1) : (1 << a.width);
    uint32_t* hist = ev_lds;
    const float* edge = (const float*)(ev_lds + nb);
    for (int b = threadIdx.x; b < nb; b += EV_THREADS) hist[b] = 0u;
    if (MODE == 0)                                 // the edges, padded with NaN (never <= a score) to 2 top - 1
        for (int t = threadIdx.x; t < 2 * a.top - 1; t += EV_THREADS)
            ev_lds[nb + t] = t < a.T ? __float_as_uint(a.edges[t]) : QNAN_BITS;
    if (threadIdx.x < 3) skip[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t nan_gen = 0u, nan_imp = 0u, ignored = 0u;
    const uint32_t mask = (1u << a.width) - 1u;
    float xs[EV_PER];                              // MODE 0: the row's scores and classes (-1: past the row's end)
    int cs[EV_PER];
    ev_walk(
        in,
        [&](long) {
#pragma unroll
            for (int i = 0; i < EV_PER; ++i) {
                xs[i] = 0.f;
                cs[i] = -1;
            }
        },
        [&](long, int i, int, float x, int c) {
            if (MODE == 0) {
                xs[i] = x;
                cs[i] = c;
            } else if (c == a.want && x == x) {
                const uint32_t bits = rank_bits(x);
                if ((uint32_t)((u64)bits >> a.hi_shift) == a.prefix) atomicAdd(&hist[(bits >> a.shift) & mask], 1u);
            }
        },
        [&](long) {
            if (MODE != 0) return;
            // pos = the number of edges <= x, a binary search of fixed length; the thread's 16 searches advance
            // together, so their LDS reads are in flight at once (a NaN compares false and stays at 0)
            int pos[EV_PER];
#pragma unroll
            for (int i = 0; i < EV_PER; ++i) pos[i] = 0;
            for (int step = a.top; step; step >>= 1) {
#pragma unroll
                for (int i = 0; i < EV_PER; ++i) {
                    const int q = pos[i] + step;   // q <= 2 top - 1: inside the padded edges
                    pos[i] = edge[q - 1] <= xs[i] ? q : pos[i];
                }
            }
#pragma unroll
            for (int i = 0; i < EV_PER; ++i) {
                const bool isnan = xs[i] != xs[i];
                if (cs[i] == 0) {
                    ++ignored;
                } else if (cs[i] > 0 && isnan) {
                    if (cs[i] == 1) ++nan_gen; else ++nan_imp;
                } else if (cs[i] > 0) {
                    atomicAdd(&hist[(cs[i] == 1 ? 0 : a.T + 1) + pos[i]], 1u);
                }
            }
        });
    if (MODE == 0) {
        if (nan_gen) atomicAdd(&skip[0], nan_gen);
        if (nan_imp) atomicAdd(&skip[1], nan_imp);
        if (ignored) atomicAdd(&skip[2], ignored);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += EV_THREADS) {
        const uint32_t v = hist[b];
        if (v == 0u) continue;
        if (MODE == 0)
            atomicAdd(b <= a.T ? a.out_a + b : a.out_b + (b - a.T - 1), (u64)v);
        else
            atomicAdd(a.out_a + b, (u64)v);
    }
    if (MODE == 0 && threadIdx.x < 3 && skip[threadIdx.x]) atomicAdd(a.skipped + threadIdx.x, (u64)skip[threadIdx.x]);
}

int check_in(const char* op, const float* scores, long ld, int P, int G, const int* row_lab, const int* col_lab,
             long lab_ld) {
    FPM_CHECK_ARG(P >= 0 && G >= 1 && ld >= G, "%s: bad sizes (P %d, G %d, ld %ld)", op, P, G, ld);
    FPM_CHECK_ARG(lab_ld == 0 || lab_ld >= G, "%s: lab_ld = %ld (0: one row of labels for all rows; else at least G = %d)",
                  op, lab_ld, G);
    FPM_CHECK_ARG(scores && row_lab && col_lab, "%s: scores, row_lab and col_lab are required", op);
    return 0;
}

unsigned slices_of(int G) { return (unsigned)(((long)G + EV_SLICE - 1) / EV_SLICE); }

// the rows of a tally launch's grid: about EV_TALLY_BLOCKS workgroups, each within EV_ROWS_MAX rows
unsigned tally_rows(int P, unsigned slices) {
    long gy = (EV_TALLY_BLOCKS + slices - 1) / slices;
    const long need = ((long)P + EV_ROWS_MAX - 1) / EV_ROWS_MAX;
    if (gy < need) gy = need;
    if (gy > P) gy = P;
    return (unsigned)(gy < 1 ? 1 : gy);
}
}  // namespace

extern "C" long fpm_mate_rank_ws_bytes(int P) { return P > 0 ? (long)P * 8 : 8; }

extern "C" int fpm_mate_rank(const float* scores, long ld, int P, int G, const int* row_lab, const int* col_lab,
                             long lab_ld, const int* own, int* mate_col, float* mate_score, int* mate_rank, void* ws,
                             long ws_bytes, void* stream) {
    if (check_in("mate_rank", scores, ld, P, G, row_lab, col_lab, lab_ld)) return 1;
    FPM_CHECK_ARG(mate_col && mate_score && mate_rank, "mate_rank: mate_col, mate_score and mate_rank are required");
    FPM_CHECK_ARG(ws && ws_bytes >= fpm_mate_rank_ws_bytes(P), "mate_rank: workspace of %ld bytes, %ld needed", ws_bytes,
                  fpm_mate_rank_ws_bytes(P));
    if (P == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, (size_t)P * 8, st) != hipSuccess || hipMemsetAsync(mate_rank, 0, (size_t)P * 4, st) != hipSuccess)
        return fpm::check_launch("fpm_mate_rank (clear)");
    const EvalIn in{scores, ld, P, G, row_lab, col_lab, lab_ld, own};
    const dim3 grid(slices_of(G), (unsigned)(P < 65535 ? P : 65535));
    hipLaunchKernelGGL(mate_max_kernel, grid, dim3(EV_THREADS), 0, st, in, (u64*)ws);
    hipLaunchKernelGGL(mate_count_kernel, grid, dim3(EV_THREADS), 0, st, in, (const u64*)ws, mate_col, mate_score,
                       mate_rank);
    return fpm::check_launch("fpm_mate_rank");
}

extern "C" int fpm_score_census(const float* scores, long ld, int P, int G, const int* row_lab, const int* col_lab,
                                long lab_ld, const int* own, const float* edges, int T, long* gen, long* imp,
                                long* skipped, void* stream) {
    if (check_in("score_census", scores, ld, P, G, row_lab, col_lab, lab_ld)) return 1;
    FPM_CHECK_ARG(T >= 1 && T <= EV_TMAX, "score_census: T = %d edges outside [1, %d]", T, EV_TMAX);
    FPM_CHECK_ARG(edges && gen && imp && skipped, "score_census: edges, gen, imp and skipped are required");
    hipStream_t st = (hipStream_t)stream;
    const size_t nb = (size_t)(T + 1) * 8;
    if (hipMemsetAsync(gen, 0, nb, st) != hipSuccess || hipMemsetAsync(imp, 0, nb, st) != hipSuccess ||
        hipMemsetAsync(skipped, 0, 24, st) != hipSuccess)
        return fpm::check_launch("fpm_score_census (clear)");
    if (P == 0) return 0;
    const EvalIn in{scores, ld, P, G, row_lab, col_lab, lab_ld, own};
    TallyArgs a{};
    a.edges = edges;
    a.T = T;
    a.top = 1;
    while (2 * a.top <= T) a.top *= 2;
    a.out_a = (u64*)gen;
    a.out_b = (u64*)imp;
    a.skipped = (u64*)skipped;
    const unsigned sl = slices_of(G);
    hipLaunchKernelGGL(tally_kernel<0>, dim3(sl, tally_rows(P, sl)), dim3(EV_THREADS), (size_t)(2 * T + 2 + 2 * a.top - 1) * 4, st, in, a);
    return fpm::check_launch("fpm_score_census");
}

extern "C" long fpm_score_select_ws_bytes(void) { return (long)EV_RADIX_BINS * 8; }

extern "C" int fpm_score_select(const float* scores, long ld, int P, int G, const int* row_lab, const int* col_lab,
                                long lab_ld, const int* own, int cls, long k, float* value, long* count, void* ws,
                                long ws_bytes, void* stream) {
    if (check_in("score_select", scores, ld, P, G, row_lab, col_lab, lab_ld)) return 1;
    FPM_CHECK_ARG(cls == 1 || cls == 2, "score_select: cls = %d (1 genuine, 2 impostor)", cls);
    FPM_CHECK_ARG(k >= 1, "score_select: k = %ld below 1", k);
    FPM_CHECK_ARG(value && count, "score_select: value and count (host) are required");
    FPM_CHECK_ARG(ws && ws_bytes >= fpm_score_select_ws_bytes(), "score_select: workspace of %ld bytes, %ld needed",
                  ws_bytes, fpm_score_select_ws_bytes());
    *count = 0;
    __builtin_memcpy(value, &QNAN_BITS, 4);
    if (P == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const EvalIn in{scores, ld, P, G, row_lab, col_lab, lab_ld, own};
    const unsigned sl = slices_of(G);
    const dim3 grid(sl, tally_rows(P, sl));
    static const int shifts[3] = {21, 10, 0}, widths[3] = {11, 11, 10};
    u64 hloc[EV_RADIX_BINS];
    uint32_t prefix = 0u;
    u64 left = (u64)k;                             // the rank wanted among the scores that match the prefix
    for (int pass = 0; pass < 3; ++pass) {
        const int bins = 1 << widths[pass];
        TallyArgs a{};
        a.want = cls;
        a.shift = shifts[pass];
        a.width = widths[pass];
        a.hi_shift = shifts[pass] + widths[pass];
        a.prefix = prefix;
        a.out_a = (u64*)ws;
        if (hipMemsetAsync(ws, 0, (size_t)bins * 8, st) != hipSuccess) return fpm::check_launch("fpm_score_select (clear)");
        hipLaunchKernelGGL(tally_kernel<1>, grid, dim3(EV_THREADS), (size_t)bins * 4, st, in, a);
        if (fpm::check_launch("fpm_score_select")) return 1;
        if (hipMemcpyAsync(hloc, ws, (size_t)bins * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fpm::check_launch("fpm_score_select (read)");
        if (pass == 0) {
            u64 n = 0;
            for (int b = 0; b < bins; ++b) n += hloc[b];
            *count = (long)n;
            if ((u64)k > n) return 0;              // value stays NaN
        }
        int d = bins - 1;
        for (; d > 0 && left > hloc[d]; --d) left -= hloc[d];
        prefix = (prefix << widths[pass]) | (uint32_t)d;
    }
    const uint32_t u = (prefix & 0x80000000u) ? (prefix & 0x7FFFFFFFu) : ~prefix;
    __builtin_memcpy(value, &u, 4);
    return 0;
}

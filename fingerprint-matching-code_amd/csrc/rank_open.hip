// Open-set 1:N search: per-group top-r fusion of match scores, and a ranked row's z-scores against its own
// impostor cohort with an accept decision.  Both kernels equal host statements bit for bit (ops.group_topr,
// ops.cohort_decide on CPU tensors), so every operation below is one rounded fp32 operation in a stated
// order.  The arithmetic goes through the helpers below, plain operators compiled with contraction off: the
// toolchain's __fadd_rn / __fmul_rn are plain operators of a header compiled with contraction on (a product and
// a sum from them fuse into an fma after inlining), and its __fsqrt_rn is the native approximation.  x / y and
// __builtin_sqrtf are the correctly rounded ones under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt.
//
// ---- group_topr: the mean of a group's r best entries ------------------------------------------------------
// The groups, their walk and gbest as rank_groups.h defines them.  For a group of c >= 1 entries
// x[0..c) (x[j] = scores[p][pos[off + j]]):
//   gscore  r' = min(r, c); the r' entries that rank first by (score descending, NaN last), x1 .. x_r';
//           s = +0.0, s = s + x1, ..., s = s + x_r' (fp32, in that order); s / fp32(r'); NaN as 0x7FC00000.
//           Entries that tie have the same value, so their order among themselves changes no bit.
//   empty   0x7FC00000, -1.
// Selection: r rounds; in each, every lane of the group's team scans its strided entries for the largest
// selection key (the ranking key over (score, j), j the entry's place in the group: unique even if a
// position repeats) strictly below the previous round's winner, an xor butterfly over (key, value) finds
// the team's, and every lane adds the winner's value.  All 64 lanes of a wave run all r rounds and reach
// every shuffle, whatever their teams' counts: an exhausted team carries key 0 and adds nothing.
//
// ---- cohort_decide: z-scores of a ranked row against its own tail ------------------------------------------
// top (P, K) fp32 contiguous, a row as fpm_rank_select returns it (descending, NaN last).  Row p's cohort:
// the non-NaN values among columns skip <= j < min(K, skip + cohort), in column order, x[0..n).
//   L(v)    64 lanes; lane t starts from +0.0 and adds v[t], v[t + 64], ... in order; then for m = 32 .. 1
//           every lane takes v + v[lane ^ m]; lane 0's value (every lane's: the addition commutes).
//   mu = L(x) / fp32(n); d_j = x_j - mu; q_j = d_j * d_j; var = L(q) / fp32(n); sigma = sqrt(var);
//   n < 2: mu = sigma = NaN.  s = max(sigma, sigma_floor), NaN if sigma is.
//   z_j = (top[p][j] - mu) / s for j < k; accept_j = (v_j >= threshold), v = z (normalize) or top; a NaN
//   never accepts.  Every NaN written is 0x7FC00000.
// One wave per row, four rows per workgroup of 256 threads; the wave compacts the window's non-NaN values
// into its 4 KB of LDS (at most 16 rounds of 64 columns: ballot and prefix count), so that the statement's
// order holds for any row, sorted or not.  Plain vector stores.
#include "rank_groups.h"
#include "fpm.h"

#pragma clang fp contract(off)

namespace {
using namespace fpm;
constexpr int COH_ROWS = 4;                        // rows (waves) per workgroup
constexpr int COH_WINDOW = 1024;                   // skip + cohort at most: 16 rounds of 64 columns

__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }
__device__ __forceinline__ float sqrt_rn(float a) { return __builtin_sqrtf(a); }
// Store v with every NaN as 0x7FC00000.  On the bits, through an integer store: a select between floats
// ("v != v ? qnan : v") may be folded away, since the compiler is free to assume which NaN an operation returned
// (it was, for the square root: sigma came out as 0xFFC00000).
__device__ __forceinline__ void store_canon(float* __restrict__ at, float v) {
    const uint32_t u = __float_as_uint(v);
    *reinterpret_cast<uint32_t*>(at) = (u & 0x7FFFFFFFu) > 0x7F800000u ? QNAN_BITS : u;
}

// One group of c entries at pos[0..c) by a team of W lanes (t: the lane's number in its team), r rounds.
// Every lane of the team leaves with the same sum, count of entries taken and best position key (0: none).
template <int W>
__device__ __forceinline__ void group_select(const float* __restrict__ row, int G, const int* __restrict__ pos, int c,
                                             int t, int r, float& sum, int& taken, u64& best) {
    u64 pb = 0ull;                                 // gbest: below every key
    for (int j = t; j < c; j += W) {
        const int q = pos[j];
        pb = group_best(pb, G, q, group_read(row, G, q));
    }
    best = team_max_u64<W>(pb);
    float s = 0.f;
    int n = 0;
    u64 prev = ~0ull;                              // above every key
    for (int round = 0; round < r; ++round) {      // r is uniform over the launch
        u64 b = 0ull;                              // below every selection key
        float bx = 0.f;
        for (int j = t; j < c; j += W) {
            const float x = group_read(row, G, pos[j]);
            const u64 key = rank_key(x, (uint32_t)j);
            if (key < prev && key > b) {
                b = key;
                bx = x;
            }
        }
#pragma unroll
        for (int m = W / 2; m >= 1; m >>= 1) {
            const u64 o = shfl_xor_u64(b, m);
            const float ox = __shfl_xor(bx, m, 64);
            if (o > b) {
                b = o;
                bx = ox;
            }
        }
        if (b != 0ull) {
            s = add_rn(s, bx);
            ++n;
        }
        prev = b;                                  // 0 once the group is exhausted: nothing is below it
    }
    sum = s;
    taken = n;
}

__device__ __forceinline__ void topr_write(float sum, int taken, u64 best, float* __restrict__ gscore,
                                           int* __restrict__ gbest) {
    if (taken <= 0 || best == 0ull) {
        store_canon(gscore, qnan());
        *gbest = -1;
        return;
    }
    *gbest = (int)rank_index(best);
    store_canon(gscore, div_rn(sum, (float)taken));
}

struct ToprGroup {
    int r;
    template <int W>
    __device__ __forceinline__ void group(const float* __restrict__ row, int G, const int* __restrict__ pos, int c, int t,
                                          bool write, int, float* __restrict__ gscore, int* __restrict__ gbest,
                                          long g) const {
        float sum;
        int taken;
        u64 best;
        group_select<W>(row, G, pos, c, t, r, sum, taken, best);
        if (write && t == 0) topr_write(sum, taken, best, gscore + g, gbest + g);
    }
};

__global__ __launch_bounds__(GRP_THREADS) void group_topr_kernel(const float* __restrict__ scores, long ld, int G,
                                                                 const int* __restrict__ grp_off, long off_ld,
                                                                 const int* __restrict__ grp_pos, long pos_ld, int S,
                                                                 int r, float* __restrict__ gscore,
                                                                 int* __restrict__ gbest) {
    group_walk(scores, ld, G, grp_off, off_ld, grp_pos, pos_ld, S, gscore, gbest, ToprGroup{r});
}

// L(v) over the n values in LDS mapped by f: lane-strided adds, then the xor butterfly
template <class F>
__device__ __forceinline__ float lane_sum(const float* __restrict__ v, int n, int lane, F f) {
    float a = 0.f;
    for (int i = lane; i < n; i += 64) a = add_rn(a, f(v[i]));
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) a = add_rn(a, __shfl_xor(a, m, 64));
    return a;
}

__global__ __launch_bounds__(COH_ROWS * 64) void cohort_decide_kernel(const float* __restrict__ top, int P, int K, int k,
                                                                      int skip, int cohort, float sigma_floor,
                                                                      int normalize, int decide, float threshold,
                                                                      float* __restrict__ z, float* __restrict__ mu_out,
                                                                      float* __restrict__ sigma_out,
                                                                      int* __restrict__ n_out, int* __restrict__ accept) {
    __shared__ float buf[COH_ROWS][COH_WINDOW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long p = (long)blockIdx.x * COH_ROWS + wave;
    const bool live = p < P;                       // a wave past the last row works on it again and stores nothing
    const float* row = top + (live ? p : (long)P - 1) * K;
    float mu = qnan(), s = qnan();
    if (normalize) {                               // uniform over the launch
        const int hi = min(K, skip + cohort);      // the window [skip, hi): at most COH_WINDOW columns
        float* x = buf[wave];
        int n = 0;
        for (int j0 = skip; j0 < hi; j0 += 64) {   // the same trips for every wave: the barrier below is reached by all
            const int j = j0 + lane;
            const float v = j < hi ? row[j] : qnan();
            const bool ok = v == v;
            const u64 mask = __ballot(ok);
            if (ok) x[n + __popcll(mask & ((1ull << lane) - 1ull))] = v;
            n += __popcll(mask);
        }
        __syncthreads();
        float sigma = qnan();
        if (n >= 2) {                              // uniform over the wave
            const float fn = (float)n;
            mu = div_rn(lane_sum(x, n, lane, [](float v) { return v; }), fn);
            const float m = mu;
            const float var = div_rn(lane_sum(x, n, lane, [m](float v) {
                                         const float d = sub_rn(v, m);
                                         return mul_rn(d, d);
                                     }), fn);
            sigma = sqrt_rn(var);
        }
        s = sigma != sigma ? qnan() : fmaxf(sigma, sigma_floor);
        if (live && lane == 0) {
            store_canon(mu_out + p, mu);
            store_canon(sigma_out + p, sigma);
            n_out[p] = n;
        }
    }
    if (!live) return;
    for (int j = lane; j < k; j += 64) {
        float v = row[j];
        if (normalize) {
            v = div_rn(sub_rn(v, mu), s);
            store_canon(z + p * k + j, v);
        }
        if (decide) accept[p * k + j] = v >= threshold ? 1 : 0;
    }
}
}  // namespace

extern "C" int fpm_group_topr(const float* scores, long ld, int P, int G, const int* grp_off, long off_ld,
                              const int* grp_pos, long pos_ld, int S, int r, float* gscore, int* gbest, void* stream) {
    return group_launch(
        "fpm_group_topr", group_topr_kernel,
        [&] {
            FPM_CHECK_ARG(r >= 1 && r <= FPM_TOPR_MAX, "group_topr: r = %d outside [1, %d]", r, FPM_TOPR_MAX);
            return 0;
        },
        scores, ld, P, G, grp_off, off_ld, grp_pos, pos_ld, S, r, gscore, gbest, stream);
}

extern "C" int fpm_cohort_decide(const float* top, int P, int K, int k, int skip, int cohort, float sigma_floor,
                                 int normalize, int decide, float threshold, float* z, float* mu, float* sigma, int* n,
                                 int* accept, void* stream) {
    FPM_CHECK_ARG(P >= 0 && K >= 1 && k >= 1 && k <= K, "cohort_decide: bad sizes (P %d, K %d, k %d)", P, K, k);
    FPM_CHECK_ARG(skip >= 0 && cohort >= 2 && (long)skip + cohort <= COH_WINDOW,
                  "cohort_decide: skip = %d, cohort = %d (skip >= 0, cohort >= 2, skip + cohort <= %d)", skip, cohort,
                  COH_WINDOW);
    FPM_CHECK_ARG((normalize == 0 || normalize == 1) && (decide == 0 || decide == 1) && (normalize || decide),
                  "cohort_decide: normalize = %d, decide = %d (each 0 or 1, not both 0)", normalize, decide);
    FPM_CHECK_ARG(!normalize || (sigma_floor > 0.f && sigma_floor <= 3.402823466e38f),
                  "cohort_decide: sigma_floor must be a positive finite number");
    FPM_CHECK_ARG(!decide || threshold == threshold, "cohort_decide: threshold is NaN");
    FPM_CHECK_ARG(top && (!normalize || (z && mu && sigma && n)) && (!decide || accept),
                  "cohort_decide: top is required, z, mu, sigma and n with normalize, accept with decide");
    FPM_CHECK_ARG(P <= 65535, "cohort_decide: at most 65535 rows per call (P %d)", P);
    if (P == 0) return 0;
    hipLaunchKernelGGL(cohort_decide_kernel, dim3((unsigned)((P + COH_ROWS - 1) / COH_ROWS)), dim3(COH_ROWS * 64), 0,
                       (hipStream_t)stream, top, P, K, k, skip, cohort, sigma_floor, normalize, decide, threshold, z, mu,
                       sigma, n, accept);
    return fpm::check_launch("fpm_cohort_decide");
}

// Per-group fusion of match scores (subject-level 1:N identification): the entries of a score row fall
// into groups (the impressions of one subject), given as CSR tables -- grp_off (S + 1 offsets) into
// grp_pos (positions into the row) -- and every (row, group) gets one fused score and the position of
// its best entry.
//
//   gbest   the position with the largest ranking key of rank.hip, (order-preserving score bits) << 32 |
//           (0xFFFFFFFF - position): the best score, ties to the lower position, NaN below every number
//           (an all-NaN group: its lowest position).
//   max     gscore = scores[p][gbest], the same bits.
//   mean    the fp32 sum of the group's entries in the order below, divided by fp32(count) with a
//           correctly rounded divide.  NaN and infinities propagate; a NaN result is written as the
//           canonical quiet NaN 0x7FC00000 (which NaN an addition returns is not a portable fact).
//   empty   gscore = 0x7FC00000, gbest = -1.
//
// Order of summation (it depends on the group's count c and the order of its positions, on nothing
// else): a team of W lanes, W = 16 for c <= 1024 and W = 64 (a whole wave) above.  Lane t starts from
// +0.0 and adds entries t, t + W, t + 2W, ... in that order; then the xor butterfly m = W/2, ..., 1:
// every lane replaces v by v + v[lane ^ m].  Lane 0's value is the sum.
//
// Grid (tiles of GRP_TILE groups, P rows), 256 threads = 16 teams of 16 lanes: team q takes the tile's
// groups q, q + 16, ...; a group over 1024 entries is left to pass 2, where wave w takes the tile's
// large groups w, w + 4, ... with all 64 lanes (S = 1 over 100 000 entries: 1563 strided rounds of one
// wave, four loads in flight).  No atomics, no scratch, no LDS, nothing shared between workgroups.
#include "fpm_common.h"
#include "fpm.h"

namespace {
constexpr int GRP_THREADS = 256;
constexpr int GRP_TEAM = 16;
constexpr int GRP_TILE = 64;                       // groups per workgroup
constexpr int GRP_WIDE = 1024;                     // counts above this take a whole wave
typedef unsigned long long u64;

// as rank.hip's rank_bits
__device__ __forceinline__ uint32_t grp_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
    return ((u64)hi << 32) | lo;
}

// One group of c entries at pos[0..c) by a team of W lanes (t: the lane's number in its team).  All 64
// lanes of the wave arrive at the butterfly, whatever their teams' counts.  A position outside [0, G)
// (the host wrapper refuses them) is read as NaN and never wins.
template <int W>
__device__ __forceinline__ void group_reduce(const float* __restrict__ row, int G, const int* __restrict__ pos, int c,
                                             int t, float& sum, u64& best) {
    float acc = 0.f;
    u64 b = 0ull;                                  // below every key: a key's position field is >= 2^31
    auto take = [&](int q, float x) {
        acc += x;
        if ((unsigned)q < (unsigned)G) {
            const u64 key = ((u64)grp_bits(x) << 32) | (0xFFFFFFFFu - (uint32_t)q);
            b = key > b ? key : b;
        }
    };
    auto read = [&](int q) { return (unsigned)q < (unsigned)G ? row[q] : __uint_as_float(0x7FC00000u); };
    int j = t;
    for (; j + 3 * W < c; j += 4 * W) {            // four loads in flight, added in order
        const int q0 = pos[j], q1 = pos[j + W], q2 = pos[j + 2 * W], q3 = pos[j + 3 * W];
        const float x0 = read(q0), x1 = read(q1), x2 = read(q2), x3 = read(q3);
        take(q0, x0);
        take(q1, x1);
        take(q2, x2);
        take(q3, x3);
    }
    for (; j < c; j += W) {
        const int q = pos[j];
        take(q, read(q));
    }
#pragma unroll
    for (int m = W / 2; m >= 1; m >>= 1) {
        acc += __shfl_xor(acc, m, 64);
        const u64 o = shfl_xor_u64(b, m);
        b = o > b ? o : b;
    }
    sum = acc;
    best = b;
}

__device__ __forceinline__ void group_write(const float* __restrict__ row, int c, float sum, u64 best, int fuse,
                                            float* __restrict__ gscore, int* __restrict__ gbest) {
    const float qnan = __uint_as_float(0x7FC00000u);
    if (c <= 0 || best == 0ull) {
        *gscore = qnan;
        *gbest = -1;
        return;
    }
    const int i = (int)(0xFFFFFFFFu - (uint32_t)best);
    *gbest = i;
    if (fuse == 0) {
        *gscore = row[i];
    } else {
        const float m = __fdiv_rn(sum, (float)c);
        *gscore = m != m ? qnan : m;
    }
}

__global__ __launch_bounds__(GRP_THREADS) void group_scores_kernel(const float* __restrict__ scores, long ld, int G,
                                                                   const int* __restrict__ grp_off, long off_ld,
                                                                   const int* __restrict__ grp_pos, long pos_ld, int S,
                                                                   int fuse, float* __restrict__ gscore,
                                                                   int* __restrict__ gbest) {
    const long p = blockIdx.y;
    const float* row = scores + p * ld;
    const int* off = grp_off + p * off_ld;
    const int* pos = grp_pos + p * pos_ld;
    float* os = gscore + p * (long)S;
    int* ob = gbest + p * (long)S;
    const long g0 = (long)blockIdx.x * GRP_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int team = threadIdx.x / GRP_TEAM, t = threadIdx.x % GRP_TEAM;
    // pass 1: a team of 16 per group of at most GRP_WIDE entries (the trip count is the same for every lane)
    for (int i = 0; i < GRP_TILE / (GRP_THREADS / GRP_TEAM); ++i) {
        const long g = g0 + team + (long)i * (GRP_THREADS / GRP_TEAM);
        int o0 = 0, c = 0;
        if (g < S) {
            o0 = off[g];
            c = off[g + 1] - o0;
        }
        const bool mine = g < S && c <= GRP_WIDE;
        float sum;
        u64 best;
        group_reduce<GRP_TEAM>(row, G, pos + o0, mine && c > 0 && o0 >= 0 ? c : 0, t, sum, best);
        if (mine && t == 0) group_write(row, o0 >= 0 ? c : 0, sum, best, fuse, os + g, ob + g);
    }
    // pass 2: a whole wave per larger group (the branch is uniform over the wave)
    for (int i = wave; i < GRP_TILE; i += GRP_THREADS / 64) {
        const long g = g0 + i;
        if (g >= S) break;
        const int o0 = off[g], c = off[g + 1] - o0;
        if (c <= GRP_WIDE || o0 < 0) continue;
        float sum;
        u64 best;
        group_reduce<64>(row, G, pos + o0, c, lane, sum, best);
        if (lane == 0) group_write(row, c, sum, best, fuse, os + g, ob + g);
    }
}
}  // namespace

extern "C" int fpm_group_scores(const float* scores, long ld, int P, int G, const int* grp_off, long off_ld,
                                const int* grp_pos, long pos_ld, int S, int fuse, float* gscore, int* gbest,
                                void* stream) {
    FPM_CHECK_ARG(P >= 0 && G >= 1 && ld >= G, "group_scores: bad sizes (P %d, G %d, ld %ld)", P, G, ld);
    FPM_CHECK_ARG(S >= 0, "group_scores: S = %d groups", S);
    FPM_CHECK_ARG(fuse == 0 || fuse == 1, "group_scores: fuse = %d (0 max, 1 mean)", fuse);
    FPM_CHECK_ARG(off_ld == 0 || off_ld >= (long)S + 1,
                  "group_scores: off_ld = %ld (0: one structure for all rows; else at least S + 1 = %ld)", off_ld,
                  (long)S + 1);
    FPM_CHECK_ARG(pos_ld >= 0 && (off_ld == 0) == (pos_ld == 0),
                  "group_scores: pos_ld = %ld with off_ld = %ld (both 0, or one structure per row)", pos_ld, off_ld);
    FPM_CHECK_ARG(scores && grp_off && grp_pos && gscore && gbest,
                  "group_scores: scores, grp_off, grp_pos, gscore and gbest are required");
    FPM_CHECK_ARG(P <= 65535, "group_scores: at most 65535 rows per call (P %d)", P);
    if (P == 0 || S == 0) return 0;
    const unsigned tiles = (unsigned)(((long)S + GRP_TILE - 1) / GRP_TILE);
    hipLaunchKernelGGL(group_scores_kernel, dim3(tiles, (unsigned)P), dim3(GRP_THREADS), 0, (hipStream_t)stream, scores,
                       ld, G, grp_off, off_ld, grp_pos, pos_ld, S, fuse, gscore, gbest);
    return fpm::check_launch("fpm_group_scores");
}

// Per-group fusion of match scores (subject-level 1:N identification): every (row, group) of the group
// walk of rank_groups.h gets one fused score and the position of its best entry.
//
//   gbest   as rank_groups.h defines it.
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
#include "rank_groups.h"
#include "fpm.h"

namespace {
using namespace fpm;

// One group of c entries at pos[0..c) by a team of W lanes (t: the lane's number in its team).  All 64
// lanes of the wave arrive at the butterfly, whatever their teams' counts.
template <int W>
__device__ __forceinline__ void group_reduce(const float* __restrict__ row, int G, const int* __restrict__ pos, int c,
                                             int t, float& sum, u64& best) {
    float acc = 0.f;
    u64 b = 0ull;                                  // below every key
    auto take = [&](int q, float x) {
        acc += x;
        b = group_best(b, G, q, x);
    };
    auto read = [&](int q) { return group_read(row, G, q); };
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
    const float nan = qnan();
    if (c <= 0 || best == 0ull) {
        *gscore = nan;
        *gbest = -1;
        return;
    }
    const int i = (int)rank_index(best);
    *gbest = i;
    if (fuse == 0) {
        *gscore = row[i];
    } else {
        const float m = __fdiv_rn(sum, (float)c);
        *gscore = m != m ? nan : m;
    }
}

struct FuseGroup {
    int fuse;
    template <int W>
    __device__ __forceinline__ void group(const float* __restrict__ row, int G, const int* __restrict__ pos, int c, int t,
                                          bool write, int cw, float* __restrict__ gscore, int* __restrict__ gbest,
                                          long g) const {
        float sum;
        u64 best;
        group_reduce<W>(row, G, pos, c, t, sum, best);
        if (write && t == 0) group_write(row, cw, sum, best, fuse, gscore + g, gbest + g);
    }
};

__global__ __launch_bounds__(GRP_THREADS) void group_scores_kernel(const float* __restrict__ scores, long ld, int G,
                                                                   const int* __restrict__ grp_off, long off_ld,
                                                                   const int* __restrict__ grp_pos, long pos_ld, int S,
                                                                   int fuse, float* __restrict__ gscore,
                                                                   int* __restrict__ gbest) {
    group_walk(scores, ld, G, grp_off, off_ld, grp_pos, pos_ld, S, gscore, gbest, FuseGroup{fuse});
}
}  // namespace

extern "C" int fpm_group_scores(const float* scores, long ld, int P, int G, const int* grp_off, long off_ld,
                                const int* grp_pos, long pos_ld, int S, int fuse, float* gscore, int* gbest,
                                void* stream) {
    return group_launch(
        "fpm_group_scores", group_scores_kernel,
        [&] {
            FPM_CHECK_ARG(fuse == 0 || fuse == 1, "group_scores: fuse = %d (0 max, 1 mean)", fuse);
            return 0;
        },
        scores, ld, P, G, grp_off, off_ld, grp_pos, pos_ld, S, fuse, gscore, gbest, stream);
}

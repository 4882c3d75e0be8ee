// The group walk shared by fpm_group_scores (rank_group.hip) and fpm_group_topr (rank_open.hip): the entries of
// a score row fall into groups, given as CSR tables -- grp_off (S + 1 offsets) into grp_pos (positions into the
// row), one structure for all rows (off_ld = pos_ld = 0) or one per row -- and every (row, group) gets one fused
// score and gbest, the position of its best entry by the ranking key of rank_key.h over (score, position): the
// best score, ties to the lower position, NaN below every number (an all-NaN group: its lowest position; an empty
// one: -1).  A position outside [0, G) (the host wrappers refuse them) reads as NaN and never is gbest.
//
// Grid (tiles of GRP_TILE groups, P rows), 256 threads.  Pass 1: 16 teams of GRP_TEAM lanes; team q takes the
// tile's groups q, q + 16, ... of at most GRP_WIDE entries, and all 64 lanes of a wave reach the per-group code
// and its shuffles, whatever their teams' counts (a team without a group runs it over 0 entries).  Pass 2: wave w
// takes the tile's larger groups w, w + 4, ... with all 64 lanes (S = 1 over 100 000 entries: 1563 strided rounds
// of one wave).  Lane 0 of the team or wave writes.  No atomics, no scratch, no LDS, nothing shared between
// workgroups.
//
// The two files differ in the per-group functor alone, and stay two translation units: rank_open.hip is compiled
// with floating-point contraction off.  ops.GROUP_TEAM and ops.GROUP_WIDE mirror GRP_TEAM and GRP_WIDE: the host
// statements sum in the order these fix.
#pragma once
#include "rank_key.h"

namespace fpm {
constexpr int GRP_THREADS = 256;
constexpr int GRP_TEAM = 16;
constexpr int GRP_TILE = 64;                       // groups per workgroup
constexpr int GRP_WIDE = 1024;                     // counts above this take a whole wave

__device__ __forceinline__ float group_read(const float* __restrict__ row, int G, int q) {
    return (unsigned)q < (unsigned)G ? row[q] : qnan();
}
// gbest's running key b (0: none yet, below every key) after the entry x at position q
__device__ __forceinline__ u64 group_best(u64 b, int G, int q, float x) {
    if ((unsigned)q < (unsigned)G) {
        const u64 key = rank_key(x, (uint32_t)q);
        b = key > b ? key : b;
    }
    return b;
}

// One workgroup's groups.  op.group<W>(row, G, pos, c, t, write, cw, gscore, gbest, g) handles one group of c
// entries at pos[0..c) by a team of W lanes (t: the lane's number in its team) and, where write holds, stores the
// group's two results at gscore[g], gbest[g] through the team's lane 0; cw is the count to report (0 for a group
// whose offset is negative).  (The addresses and the lane test are left to the functor, after its reduction:
// formed before it, they cost the kernels two registers.)
template <class Op>
__device__ __forceinline__ void group_walk(const float* __restrict__ scores, long ld, int G,
                                           const int* __restrict__ grp_off, long off_ld,
                                           const int* __restrict__ grp_pos, long pos_ld, int S,
                                           float* __restrict__ gscore, int* __restrict__ gbest, Op op) {
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
        op.template group<GRP_TEAM>(row, G, pos + o0, mine && c > 0 && o0 >= 0 ? c : 0, t, mine, o0 >= 0 ? c : 0, os,
                                    ob, g);
    }
    // pass 2: a whole wave per larger group (the branch is uniform over the wave)
    for (int i = wave; i < GRP_TILE; i += GRP_THREADS / 64) {
        const long g = g0 + i;
        if (g >= S) break;
        const int o0 = off[g], c = off[g + 1] - o0;
        if (c <= GRP_WIDE || o0 < 0) continue;
        op.template group<64>(row, G, pos + o0, c, lane, true, c, os, ob, g);
    }
}

typedef void (*group_kernel_t)(const float*, long, int, const int*, long, const int*, long, int, int, float*, int*);

// The argument checks and the launch of both entry points; the messages name the operation, the entry point
// without its "fpm_"; check_arg checks the operation's own argument (fuse, r) in its place among the others.
template <class CheckArg>
int group_launch(const char* entry, group_kernel_t kernel, CheckArg&& check_arg, const float* scores, long ld, int P,
                 int G, const int* grp_off, long off_ld, const int* grp_pos, long pos_ld, int S, int arg, float* gscore,
                 int* gbest, void* stream) {
    const char* op = entry + 4;
    FPM_CHECK_ARG(P >= 0 && G >= 1 && ld >= G, "%s: bad sizes (P %d, G %d, ld %ld)", op, P, G, ld);
    FPM_CHECK_ARG(S >= 0, "%s: S = %d groups", op, S);
    if (check_arg()) return 1;
    FPM_CHECK_ARG(off_ld == 0 || off_ld >= (long)S + 1,
                  "%s: off_ld = %ld (0: one structure for all rows; else at least S + 1 = %ld)", op, off_ld,
                  (long)S + 1);
    FPM_CHECK_ARG(pos_ld >= 0 && (off_ld == 0) == (pos_ld == 0),
                  "%s: pos_ld = %ld with off_ld = %ld (both 0, or one structure per row)", op, pos_ld, off_ld);
    FPM_CHECK_ARG(scores && grp_off && grp_pos && gscore && gbest,
                  "%s: scores, grp_off, grp_pos, gscore and gbest are required", op);
    FPM_CHECK_ARG(P <= 65535, "%s: at most 65535 rows per call (P %d)", op, P);
    if (P == 0 || S == 0) return 0;
    const unsigned tiles = (unsigned)(((long)S + GRP_TILE - 1) / GRP_TILE);
    hipLaunchKernelGGL(kernel, dim3(tiles, (unsigned)P), dim3(GRP_THREADS), 0, (hipStream_t)stream, scores, ld, G,
                       grp_off, off_ld, grp_pos, pos_ld, S, arg, gscore, gbest);
    return check_launch(entry);
}
}  // namespace fpm

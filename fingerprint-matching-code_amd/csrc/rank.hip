// Per-probe top-k ranking of match scores (1:N identification): for every row of scores (P, G) the k
// best gallery entries in descending score order, ties to the lower index, NaN after every number
// (NaNs among themselves by index).
//
// Every element gets its ranking key (rank_key.h), unique per element, so the ranking is "the k
// largest keys" with no tie logic: round j takes the largest key below round j-1's.  One workgroup
// per row streams the row once per round (k <= 128; the row of one probe is a few KB and stays in
// L2); wave max-reduce on __shfl_xor, the four waves join through LDS.  Deterministic: a max over
// unique keys has one answer.
#include "rank_key.h"
#include "fpm.h"

namespace {
using namespace fpm;
constexpr int RANK_THREADS = 256;

__global__ __launch_bounds__(RANK_THREADS) void rank_topk_kernel(const float* __restrict__ scores, long ld, int G, int k,
                                                                 int* __restrict__ top_idx,
                                                                 float* __restrict__ top_score) {
    __shared__ u64 part[2][RANK_THREADS / 64];
    const float* row = scores + (long)blockIdx.x * ld;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 prev = ~0ull;                          // above every key
    for (int j = 0; j < k; ++j) {
        u64 best = 0ull;                       // below every key
        for (int i = threadIdx.x; i < G; i += RANK_THREADS) {
            const u64 key = rank_key(row[i], (uint32_t)i);
            if (key < prev && key > best) best = key;
        }
        best = team_max_u64<64>(best);
        if (lane == 0) part[j & 1][wave] = best;
        __syncthreads();                       // part[] alternates, so one barrier per round suffices
        u64 m = part[j & 1][0];
#pragma unroll
        for (int w = 1; w < RANK_THREADS / 64; ++w) m = part[j & 1][w] > m ? part[j & 1][w] : m;
        prev = m;
        if (threadIdx.x == 0) {
            const int i = (int)rank_index(m);
            top_idx[(long)blockIdx.x * k + j] = i;
            top_score[(long)blockIdx.x * k + j] = row[i];
        }
    }
}
}  // namespace

extern "C" int fpm_rank_topk(const float* scores, long ld, int P, int G, int k, int* top_idx, float* top_score,
                             void* stream) {
    FPM_CHECK_ARG(P >= 0 && G >= 1 && ld >= G, "rank_topk: bad sizes (P %d, G %d, ld %ld)", P, G, ld);
    FPM_CHECK_ARG(k >= 1 && k <= 128 && k <= G, "rank_topk: k = %d outside [1, min(G, 128)]", k);
    FPM_CHECK_ARG(scores && top_idx && top_score, "rank_topk: scores, top_idx and top_score are required");
    if (P == 0) return 0;
    hipLaunchKernelGGL(rank_topk_kernel, dim3((unsigned)P), dim3(RANK_THREADS), 0, (hipStream_t)stream, scores, ld, G, k,
                       top_idx, top_score);
    return fpm::check_launch("fpm_rank_topk");
}

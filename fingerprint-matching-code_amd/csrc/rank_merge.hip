// Merge of sorted candidate lists (a gallery spread over several devices: every shard's shortlist, carried
// to one device, merged into the global shortlist).  Row p holds L = list_off[S] candidates, a score and an
// id each; list t is the columns [list_off[t], list_off[t + 1]).  key(c) = rank_key(score, id): the
// ranking key of rank_key.h with the candidate's id (a global entry number) in place of its column, so a
// tie between lists goes to the lower id wherever the two candidates sit in the row.
//
// Precondition (what fpm_rank_select over a shard plus an ascending id table gives): every list is strictly
// descending by key, and the ids of a row are distinct, so keys are unique.
//
// Merge by ranking: the output slot of candidate c is the number of keys greater than key(c), summed over
// the lists: one binary search per list (in c's own list it finds c's place).  A candidate whose slot is
// below k writes itself there.  No sort, no atomics, nothing shared between workgroups: one answer whatever
// the schedule.  Only the first min(len, k) candidates of a list can matter (a later one is beaten by k of
// its own list; a count of k or more in one list already puts a candidate out), so those alone are staged,
// searched and ranked.
//
// One workgroup of 1024 threads per row.  The keys live in LDS, 8 bytes a column: 4 KB for 8 lists of 64,
// 128 KB at the limit (16 lists of 1024), where one workgroup fills a CU; a binary search is ten dependent
// reads, LDS latency each instead of an L2 round trip.  The list offsets come by value in the kernel
// arguments (checked on the host) and are copied to LDS for indexing.
//
// For data that breaks the precondition the kernel still ends and stays inside its buffers: a search is
// bounded by its list, and a slot is used only below k.  Slots may then be written twice or not at all.
#include "rank_key.h"
#include "fpm.h"

namespace {
using namespace fpm;
constexpr int MG_THREADS = 1024;

struct MergeLists {
    int off[FPM_TOPK_MERGE_SMAX + 1];
};

__global__ __launch_bounds__(MG_THREADS) void topk_merge_kernel(const float* __restrict__ score,
                                                                const int* __restrict__ id, long ld, MergeLists lists,
                                                                int S, int k, int* __restrict__ top_id,
                                                                float* __restrict__ top_score,
                                                                int* __restrict__ top_col) {
    extern __shared__ u64 keys[];                  // one per column of the row; only the staged ones are read
    __shared__ int off[FPM_TOPK_MERGE_SMAX + 1];
    const long p = blockIdx.x;
    const float* rs = score + p * ld;
    const int* ri = id + p * ld;
    if (threadIdx.x <= S) off[threadIdx.x] = lists.off[threadIdx.x];
    __syncthreads();
    // work item w: candidate j of list t, j < min(len_t, k)
    const int items = S * k;
    for (int w = threadIdx.x; w < items; w += MG_THREADS) {
        const int t = w / k, j = w - t * k;
        const int c = off[t] + j;
        if (c < off[t + 1]) keys[c] = rank_key(rs[c], (uint32_t)ri[c]);
    }
    __syncthreads();
    for (int w = threadIdx.x; w < items; w += MG_THREADS) {
        const int t = w / k, j = w - t * k;
        const int c = off[t] + j;
        if (c >= off[t + 1]) continue;
        const u64 key = keys[c];
        int slot = 0;
        for (int u = 0; u < S && slot < k; ++u) {
            // the number of keys above mine among list u's first k: its lists descend, so the first place
            // whose key is not above mine
            const int b = off[u];
            int lo = b, hi = min(off[u + 1], b + k);
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (keys[mid] > key) lo = mid + 1;
                else hi = mid;
            }
            slot += lo - b;
        }
        if (slot < k) {
            const long o = p * (long)k + slot;
            top_id[o] = ri[c];
            reinterpret_cast<uint32_t*>(top_score)[o] = __float_as_uint(rs[c]);      // the same bits, NaNs too
            top_col[o] = c;
        }
    }
}
}  // namespace

extern "C" int fpm_topk_merge(const float* score, const int* id, long ld, int P, const int* list_off, int S, int k,
                              int* top_id, float* top_score, int* top_col, void* stream) {
    FPM_CHECK_ARG(S >= 1 && S <= FPM_TOPK_MERGE_SMAX, "topk_merge: S = %d lists outside [1, %d]", S,
                  FPM_TOPK_MERGE_SMAX);
    FPM_CHECK_ARG(list_off, "topk_merge: list_off (S + 1 host offsets) is required");
    FPM_CHECK_ARG(list_off[0] == 0, "topk_merge: list_off must start at 0 (got %d)", list_off[0]);
    MergeLists lists;
    for (int t = 0; t <= FPM_TOPK_MERGE_SMAX; ++t) lists.off[t] = 0;
    for (int t = 0; t < S; ++t) {
        const long len = (long)list_off[t + 1] - list_off[t];
        FPM_CHECK_ARG(len >= 0 && len <= FPM_RANK_SELECT_KMAX,
                      "topk_merge: list %d holds %ld candidates (offsets must not fall; at most %d a list)", t, len,
                      FPM_RANK_SELECT_KMAX);
        lists.off[t + 1] = list_off[t + 1];
    }
    const int L = list_off[S];
    FPM_CHECK_ARG(L >= 1, "topk_merge: every list is empty");
    FPM_CHECK_ARG(P >= 0 && P <= 65535, "topk_merge: P = %d rows outside [0, 65535]", P);
    FPM_CHECK_ARG(ld >= L, "topk_merge: row stride ld = %ld below the row's %d candidates", ld, L);
    FPM_CHECK_ARG(k >= 1 && k <= L && k <= FPM_RANK_SELECT_KMAX, "topk_merge: k = %d outside [1, min(L = %d, %d)]", k,
                  L, FPM_RANK_SELECT_KMAX);
    FPM_CHECK_ARG(score && id && top_id && top_score && top_col,
                  "topk_merge: score, id, top_id, top_score and top_col are required");
    if (P == 0) return 0;
    const size_t lds = (size_t)L * sizeof(u64);
    if (lds > 65536 &&
        hipFuncSetAttribute((const void*)topk_merge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess) {
        (void)hipGetLastError();
        fpm::set_error("topk_merge: the device refuses %zu bytes of LDS per workgroup", lds);
        return 1;
    }
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)P), dim3(MG_THREADS), lds, (hipStream_t)stream, score, id, ld,
                       lists, S, k, top_id, top_score, top_col);
    return fpm::check_launch("fpm_topk_merge");
}

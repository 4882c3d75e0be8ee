// The probe side of a coarse-score launch (coarse.hip, coarse_wide.hip, coarse_stream.hip), a
// compile-time choice: one probe for every pair of the launch, or a pair list, in which the probe of
// pair b is graph qidx[b] of a second ragged fp32 row store.  The kernels differ in this lookup alone.
// Both instantiations share one argument list (the pair list's two extra pointers come last and are
// never read by the one-probe code, which keeps its __restrict__ probe pointer), so the one-probe
// kernels keep the registers and spills they had; the fused ones compile to the very same instructions.
#pragma once
#include <vector>

#include "coarse_tile.h"
#include "fpm_common.h"

namespace fpm {
// Pair b's probe rows and keypoint count.  One probe (PAIRS false): ypq is the probe's (n0, 768) rows and
// n0q its keypoint count, as ever; qrow_off and qidx are not read.  A pair list: ypq is the probe row
// store yq (sum n_q, 768), graph q at rows [qrow_off[q], qrow_off[q + 1]), n0q its graph count Q, and the
// probe of pair b is graph qidx[b].  b is uniform over the workgroup, so the lookup is two scalar loads,
// as idx[b] / row_off[g] are, and yp and n0 stay scalar.  A qidx outside [0, Q) gives n0 = 0, which the
// kernel's bound check refuses (as it refuses n0 over its box) before yp is read.
template <bool PAIRS>
__device__ __forceinline__ void coarse_probe_of(const float* ypq, int n0q, const long* qrow_off, const int* qidx, int b,
                                                const float*& yp, int& n0) {
    if constexpr (PAIRS) {
        const int q = qidx[b];
        long q0 = 0, nql = 0;
        if (q >= 0 && q < n0q) {
            q0 = qrow_off[q];
            nql = qrow_off[q + 1] - q0;
        }
        n0 = nql >= 1 && nql <= 0x7fffffffL ? (int)nql : 0;
        yp = ypq + q0 * 768;
    } else {
        yp = ypq;
        n0 = n0q;
    }
}

// Host side of a pair-list entry point: the smallest and largest keypoint count among the probes that
// qidx[0 .. B) names, so that a probe outside the kernel's box is refused by name before the launch, as
// the one-probe entry points refuse their n0.  qidx and qrow_off are device memory: they are read back
// on ``stream`` (B int32 + Q + 1 int64, one wait per launch).  A qidx outside [0, Q) is skipped: like a
// bad idx it is the caller's to check, and the kernel gives that pair NaN.  Returns 1 on a HIP error.
inline int coarse_pairs_probe_range(const long* qrow_off, const int* qidx, int Q, int B, void* stream, long& lo,
                                    long& hi) {
    std::vector<long> off((size_t)Q + 1);
    std::vector<int> qi((size_t)B);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemcpyAsync(off.data(), qrow_off, off.size() * sizeof(long), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(qi.data(), qidx, qi.size() * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        set_error("coarse_pairs: reading qrow_off / qidx back failed");
        return 1;
    }
    lo = 1;
    hi = 1;
    bool any = false;
    for (int b = 0; b < B; ++b) {
        if (qi[b] < 0 || qi[b] >= Q) continue;
        const long n = off[qi[b] + 1] - off[qi[b]];
        lo = any && lo < n ? lo : n;
        hi = any && hi > n ? hi : n;
        any = true;
    }
    return 0;
}

// The host side of the C entry points, once for the three kernels.  K is a kernel's traits: its op names
// (``score_op``, ``pairs_op``) as the messages spell them, its bound (``bound``, ``nmax``), and
// (YT: float, bf16_t or coarse::fp8_t; y: coarse::EntryRows<YT>::host, a pointer or the fp8 rows' pair)
//     K::launch<YT, PAIRS>(what, y, row_off, idx, G, B, ypq, n0q, qrow_off, qidx, n0max, coef, iters, tau,
//                          score, ws, ws_bytes, stream)
// which checks the kernel's workspace (n0max: the largest probe of the launch), sizes the grid and
// launches.  ws / ws_bytes are null / 0 for a kernel without a workspace.
template <class K, typename YT>
int coarse_score_entry(const char* what, typename coarse::EntryRows<YT>::host y, const long* row_off, const int* idx,
                       int G, int B, const float* yp, int n0, const float* coef, int iters, float tau, float* score,
                       void* ws, long ws_bytes, void* stream) {
    FPM_CHECK_ARG(G > 0 && B >= 0, "%s: bad sizes (G %d, B %d)", K::score_op, G, B);
    FPM_CHECK_ARG(n0 >= 1 && n0 <= K::nmax, "%s: probe of %d keypoints outside [1, %s = %d]", K::score_op, n0, K::bound,
                  K::nmax);
    FPM_CHECK_ARG(iters >= 0 && tau > 0.f, "%s: iters >= 0 and tau > 0 required", K::score_op);
    FPM_CHECK_ARG(coarse::rows_given(y) && row_off && idx && yp && coef && score,
                  "%s: y (fp8 rows: and their scales), row_off, idx, yp, coef and score are required", K::score_op);
    if (B == 0) return 0;
    return K::template launch<YT, false>(what, y, row_off, idx, G, B, yp, n0, nullptr, nullptr, n0, coef, iters, tau,
                                         score, ws, ws_bytes, stream);
}

// the pair list: the one-probe refusals, the probe sizes read back from the device
template <class K, typename YT>
int coarse_pairs_entry(const char* what, typename coarse::EntryRows<YT>::host y, const long* row_off, const int* idx,
                       int G, int B, const float* yq, const long* qrow_off, const int* qidx, int Q, const float* coef,
                       int iters, float tau, float* score, void* ws, long ws_bytes, void* stream) {
    FPM_CHECK_ARG(G > 0 && Q > 0 && B >= 0, "%s: bad sizes (G %d, Q %d, B %d)", K::pairs_op, G, Q, B);
    FPM_CHECK_ARG(iters >= 0 && tau > 0.f, "%s: iters >= 0 and tau > 0 required", K::pairs_op);
    FPM_CHECK_ARG(coarse::rows_given(y) && row_off && idx && yq && qrow_off && qidx && coef && score,
                  "%s: y (fp8 rows: and their scales), row_off, idx, yq, qrow_off, qidx, coef and score are required",
                  K::pairs_op);
    if (B == 0) return 0;
    long lo, hi;
    if (coarse_pairs_probe_range(qrow_off, qidx, Q, B, stream, lo, hi)) return 1;
    FPM_CHECK_ARG(lo >= 1 && hi <= K::nmax, "%s: probe of %ld keypoints outside [1, %s = %d]", K::pairs_op,
                  hi > K::nmax ? hi : lo, K::bound, K::nmax);
    return K::template launch<YT, true>(what, y, row_off, idx, G, B, yq, Q, qrow_off, qidx, (int)hi, coef, iters, tau,
                                        score, ws, ws_bytes, stream);
}
}  // namespace fpm

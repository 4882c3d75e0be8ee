// The coarse 1:N score of coarse.hip (same definition, see there) for boxes of up to 256 keypoints:
//
//     score = sum_{i < n0, j < n_g} P_ij Kp_ij / min(n0, n_g),
//     Kp = softplus(a b^T) - 0.5,  a = bf16(y_p o c),  b = bf16(y_g),
//     P  = Sinkhorn(Kp; dummy rows, iters, tau)          (pygmtools' log-domain Sinkhorn).
//
// A 256 x 256 fp32 block is 256 KB, over the CU's 160 KB of LDS, so here L lives in registers, in the
// MFMA accumulators' own layout: one workgroup of 512 threads per pair, 8 waves in a 4 (rows) x 2
// (columns) grid, a wave's 64 x 128 part of the block in 4 x 8 fragments of 16 x 16 = 128
// accumulators per thread (two waves per SIMD: 256 registers each).
//   1. a b^T on v_mfma_f32_16x16x32_bf16, rows = the smaller side (the Sinkhorn's orientation).  The
//      fp32 rows come from global memory, are scaled (probe side) and rounded to bf16 on the way
//      into LDS; K = 768 in 24 tiles of 32 (the prefetch registers sit beside the 128 accumulators),
//      two LDS buffers, one barrier per tile, the next tile's loads in flight under the MFMAs.
//   2. The epilogue (softplus on the native exp2 / log2, see softplus_native) parks Kp (fp32, 0
//      outside the block) in the workgroup's own 256 KB slot of a device workspace, each thread its
//      own accumulators (16 B per lane, coalesced; the same thread reads them back, so nothing is
//      handed between threads), and turns the accumulators into L = Kp / tau in log2 units, -inf
//      outside the block.
//   3. The Sinkhorn updates L in place (L -= lse).  A row's lse: in-thread over the wave's 8 column
//      fragments, a 16-lane DPP tree, then the two column waves' (max, sum) partials through LDS,
//      merged in wave order.  A column's lse: in-thread over r and the 4 row fragments, the four
//      lane groups (v_permlane16/32_swap), then the four row waves' partials through LDS, merged in
//      wave order, then the dummy rows' term.  The nd = C - R dummy rows are one vector of
//      multiplicity nd in LDS.  Rows and columns outside the block hold -inf and get lse = 0.
//   4. sum exp2(L) Kp over each thread's accumulator positions (Kp read back from the slot), wave
//      sums (DPP), the eight waves through LDS in wave order; 4 bytes out.
// The grid is persistent: min(B, 256) workgroups, workgroup w takes pairs w, w + grid, ...; the
// workspace is one slot per workgroup, at most 64 MB whatever B.  Every order of summation is fixed
// by the pair alone, so an entry's score is bit-identical whatever else shares the launch and
// whichever workgroup computes it.  No spinning, no exchange between workgroups.  LDS: 93.0 KB per
// workgroup, one workgroup per CU.
#include "fpm_common.h"
#include "coarse_probe.h"
#include "coarse_tile.h"
#include "fpm.h"

namespace {
constexpr int WN = FPM_COARSE_WIDE_NMAX;     // 256
constexpr int WT = 512;                      // threads
constexpr int WK = 768;                      // channels
constexpr int WBK = 32;                      // K tile
constexpr int WROW = 80;                     // bytes per operand row in LDS: 32 bf16 + 16 B pad
constexpr int WTILE = WN * WROW;             // one side's tile
constexpr int WBUF = 2 * WTILE;              // both sides
constexpr int WGRID = 256;                   // workgroups at most (one per CU)
constexpr int FM = 4, FN = 8;                // a wave's fragments: 64 rows x 128 columns
constexpr long SLOT_FLOATS = (long)WN * WN;  // Kp of one pair
// LDS after the two tile buffers: row partials [2][256] x (max, sum), column partials [4][256] x
// (max, sum), the dummy vector [256], the wave sums [8]
constexpr int RED_FLOATS = 4 * WN + 8 * WN + WN + 8;
constexpr int WLDS = 2 * WBUF + RED_FLOATS * 4;

using namespace fpm::coarse;
// a K tile: 4 float4 (256 rows) or 2 vectors of 8 bf16 per thread (coarse_tile.h)
using KTile = Tile<WT, WBK, WROW>;

// This thread's coordinates from a thread index the optimiser cannot see through.  The kernel is one
// loop over pairs; every index and address below is invariant in it, and hoisted out of it they
// would all be live at once beside the 128 accumulators (spills).  Each phase takes a fresh copy, so
// its few address registers are computed where they are used and die with the phase.
struct Pos {
    int tid, lane, fr, fq;
};
__device__ __forceinline__ Pos fresh_pos() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return Pos{t, t & 63, t & 15, (t >> 4) & 3};
}

// YT: the entry rows' type, float (rounded on the way into LDS), bf16_t (rounded at enrolment) or fp8_t
// (e4m3 with a row scale, quantised at enrolment and dequantised, exactly, on the way into LDS); the
// probe side and everything after the tile store are the same code, so are the bits.  PAIRS: the probe
// of pair b comes from a second row store (a pair list: coarse_probe.h), looked up per pair of the
// persistent walk; that lookup is the only code that differs
template <typename YT, bool PAIRS>
__global__ __launch_bounds__(WT) void coarse_score_wide_kernel(typename EntryRows<YT>::arg y,
                                                               const long* __restrict__ row_off,
                                                               const int* __restrict__ idx, int G, int B,
                                                               const float* __restrict__ ypq, int n0q,
                                                               const float* __restrict__ coef, int iters, float tau,
                                                               float* __restrict__ score, float* __restrict__ ws,
                                                               const long* __restrict__ qrow_off,
                                                               const int* __restrict__ qidx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wlds[];
    float* rm = (float*)(wlds + 2 * WBUF);   // [2][256] row partial maxima (per column wave)
    float* rs = rm + 2 * WN;                 // [2][256] row partial sums
    float* cm = rs + 2 * WN;                 // [4][256] column partial maxima (per row wave)
    float* cs = cm + 4 * WN;                 // [4][256] column partial sums
    float* D = cs + 4 * WN;                  // [256] the dummy rows' vector
    float* red = D + WN;                     // [8] wave sums

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar: wave-uniform branches
    const int wm = wave >> 1, wn = wave & 1;
    f32x4_t* slot = (f32x4_t*)(ws + (long)blockIdx.x * SLOT_FLOATS);

    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const int g = idx[b];
        long r0 = 0, ngl = 0;
        if (g >= 0 && g < G) {
            r0 = row_off[g];
            ngl = row_off[g + 1] - r0;
        }
        const float* yp;
        int n0;
        fpm::coarse_probe_of<PAIRS>(ypq, n0q, qrow_off, qidx, b, yp, n0);
        // the wrapper checks both on the host; never read outside y, never index past the 256 x 256 box
        if (ngl < 1 || ngl > WN || n0 < 1 || n0 > WN) {   // uniform over the workgroup
            if (threadIdx.x == 0) score[b] = __uint_as_float(0x7FC00000u);
            continue;
        }
        const int ng = (int)ngl;
        // the Sinkhorn works on the transpose when n0 > n_g: its rows are the smaller side
        const bool tr = n0 > ng;
        const int R = tr ? ng : n0, C = tr ? n0 : ng;
        constexpr bool F32 = sizeof(YT) == 4, F8 = sizeof(YT) == 1;
        const auto ye = y + r0 * WK;                   // the entry's rows
        const float* xa = nullptr;                       // rows side (MFMA A)
        const float* xb = nullptr;                       // columns side (MFMA B)
        if constexpr (F32) {
            xa = tr ? ye : yp;
            xb = tr ? yp : ye;
        }
        const float* cf = coef + (long)b * WK;
        const int nd = C - R;                    // dummy rows (dummy_row = True)
        // a wave whose 64 x 128 part lies wholly outside the block holds nothing: it only reports empty
        // partials and meets the barriers
        const bool live = wm * 64 < R && wn * 128 < C;
        const float fnd = (float)nd;

        f32x4_t L[FM][FN];
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) L[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

        {   // a b^T
            const Pos p = fresh_pos();
            const int tid = p.tid, fr = p.fr, fq = p.fq, c4 = 4 * (tid & 7);
            const float4 one = make_float4(1.f, 1.f, 1.f, 1.f);
            float4 ra[4], rb[4], sc;
            uint4 re[2];                                 // bf16 entry rows: ra is the probe's tile, re the entry's
            uint2 r8[2];                                 // fp8 entry rows: r8 the entry's tile, s8 its rows' scales
            float s8[2];
            if constexpr (F32) {
                KTile::load(xa, R, 0, 0, tid, ra);
                KTile::load(xb, C, 0, 0, tid, rb);
            } else if constexpr (F8) {
                KTile::load(yp, n0, 0, 0, tid, ra);
                KTile::load8(ye, ng, 0, 0, tid, r8);
                KTile::load8_scale(ye, ng, 0, tid, s8);
            } else {
                KTile::load(yp, n0, 0, 0, tid, ra);
                KTile::load16(ye, ng, 0, 0, tid, re);
            }
            sc = *(const float4*)(cf + c4);
            for (int kt = 0; kt < WK / WBK; ++kt) {
                unsigned char* At = wlds + (kt & 1) * WBUF;
                unsigned char* Bt = At + WTILE;
                if constexpr (F32) {
                    KTile::store(At, tid, ra, tr ? one : sc);
                    KTile::store(Bt, tid, rb, tr ? sc : one);
                } else if constexpr (F8) {
                    KTile::store(tr ? Bt : At, tid, ra, sc);
                    KTile::store8(tr ? At : Bt, tid, r8, s8);
                } else {                                 // the entry is the MFMA's A when transposed, B otherwise
                    KTile::store(tr ? Bt : At, tid, ra, sc);
                    KTile::store16(tr ? At : Bt, tid, re);
                }
                // one barrier per tile: the other buffer was last read before the previous barrier
                __syncthreads();
                if (kt + 1 < WK / WBK) {
                    if constexpr (F32) {
                        KTile::load(xa, R, 0, (kt + 1) * WBK, tid, ra);
                        KTile::load(xb, C, 0, (kt + 1) * WBK, tid, rb);
                    } else if constexpr (F8) {
                        KTile::load(yp, n0, 0, (kt + 1) * WBK, tid, ra);
                        KTile::load8(ye, ng, 0, (kt + 1) * WBK, tid, r8);
                    } else {
                        KTile::load(yp, n0, 0, (kt + 1) * WBK, tid, ra);
                        KTile::load16(ye, ng, 0, (kt + 1) * WBK, tid, re);
                    }
                    sc = *(const float4*)(cf + (kt + 1) * WBK + c4);
                }
                bf16x8_t a[FM];
#pragma unroll
                for (int f = 0; f < FM; ++f)
                    a[f] = *(const bf16x8_t*)(At + (wm * 64 + f * 16 + fr) * WROW + fq * 16);
#pragma unroll
                for (int fn = 0; fn < FN; ++fn) {
                    if (wn * 128 + fn * 16 >= C) continue;       // fragments past the block: wave-uniform
                    const bf16x8_t bb = *(const bf16x8_t*)(Bt + (wn * 128 + fn * 16 + fr) * WROW + fq * 16);
#pragma unroll
                    for (int fm = 0; fm < FM; ++fm) {
                        if (wm * 64 + fm * 16 >= R) continue;
                        L[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[fm], bb, L[fm][fn], 0, 0, 0);
                    }
                }
            }
        }

        {   // Kp into the slot (0 outside the block), L = Kp / tau in log2 units (-inf outside)
            const Pos p = fresh_pos();
            const int tid = p.tid, fr = p.fr, fq = p.fq;
            if (live) {
#pragma unroll
                for (int fm = 0; fm < FM; ++fm)
#pragma unroll
                    for (int fn = 0; fn < FN; ++fn) {
                        f32x4_t kp4;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int i = wm * 64 + fm * 16 + 4 * fq + r, j = wn * 128 + fn * 16 + fr;
                            float kp = 0.f, l = -INFINITY;
                            if (i < R && j < C) {
                                kp = softplus_native(L[fm][fn][r]) - 0.5f;
                                l = (kp / tau) * fpm::LOG2E_F;
                            }
                            kp4[r] = kp;
                            L[fm][fn][r] = l;
                        }
                        slot[(fm * FN + fn) * WT + tid] = kp4;
                        __builtin_amdgcn_sched_barrier(0);       // one fragment's temporaries at a time
                    }
            }
            if (nd > 0 && tid < C) D[tid] = -100.f * fpm::LOG2E_F;
        }
        __syncthreads();

        // two steps per turn, so the accumulators are carried by one loop, not merged from two branches
        for (int it = 0; it < iters; it += 2) {
            {   // rows: this thread's 16 rows over its wave's 128 columns ...
                const Pos p = fresh_pos();
                const int lane = p.lane, fr = p.fr, fq = p.fq;
#pragma unroll
                for (int fm = 0; fm < FM; ++fm)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float m = -INFINITY, s = 0.f;
                        if (live) {
                            m = L[fm][0][r];
#pragma unroll
                            for (int fn = 1; fn < FN; ++fn) m = fmaxf(m, L[fm][fn][r]);
                            m = row16_max(m);
                            const float mf = finite_max(m);
#pragma unroll
                            for (int fn = 0; fn < FN; ++fn) s += fpm::fast_exp2(L[fm][fn][r] - mf);
                            s = fpm::row16_sum(s);
                        }
                        if (fr == 0) {
                            const int i = wm * 64 + fm * 16 + 4 * fq + r;
                            rm[wn * WN + i] = m;
                            rs[wn * WN + i] = s;
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                if (wave == 0 && nd > 0) {
                    // the dummy rows: one row over all C columns, 4 per lane
                    float x[4];
                    float m = -INFINITY;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = lane + 64 * q;
                        x[q] = c < C ? D[c] : -INFINITY;
                        m = fmaxf(m, x[q]);
                    }
                    m = fpm::warp_max(m);                      // finite: column 0 exists
                    float s = 0.f;
#pragma unroll
                    for (int q = 0; q < 4; ++q) s += fpm::fast_exp2(x[q] - m);
                    s = fpm::warp_sum(s);
                    const float lse = m + fpm::fast_log2(s);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = lane + 64 * q;
                        if (c < C) D[c] = x[q] - lse;
                    }
                }
            }
            __syncthreads();
            if (live) {   // ... then the two column waves' partials, in wave order
                const Pos p = fresh_pos();
                const int fq = p.fq;
#pragma unroll
                for (int fm = 0; fm < FM; ++fm)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = wm * 64 + fm * 16 + 4 * fq + r;
                        const float m0 = rm[i], m1 = rm[WN + i];
                        const float mm = fmaxf(m0, m1), mf = finite_max(mm);
                        const float t = rs[i] * fpm::fast_exp2(m0 - mf) + rs[WN + i] * fpm::fast_exp2(m1 - mf);
                        const float lse = mm == -INFINITY ? 0.f : mm + fpm::fast_log2(t);
#pragma unroll
                        for (int fn = 0; fn < FN; ++fn) L[fm][fn][r] -= lse;
                        __builtin_amdgcn_sched_barrier(0);
                    }
            }
            if (it + 1 >= iters) break;              // uniform: iters is odd and this was its last step

            // columns: this thread's 8 columns over its 16 rows, the four lane groups ...
            float dj[FN];
            {
                const Pos p = fresh_pos();
                const int fr = p.fr, fq = p.fq;
#pragma unroll
                for (int fn = 0; fn < FN; ++fn) {
                    float m = -INFINITY, s = 0.f;
                    if (live) {
#pragma unroll
                        for (int fm = 0; fm < FM; ++fm)
#pragma unroll
                            for (int r = 0; r < 4; ++r) m = fmaxf(m, L[fm][fn][r]);
                        m = fpm::pair32_max(fpm::pair16_max(m));
                        const float mf = finite_max(m);
#pragma unroll
                        for (int fm = 0; fm < FM; ++fm)
#pragma unroll
                            for (int r = 0; r < 4; ++r) s += fpm::fast_exp2(L[fm][fn][r] - mf);
                        s = fpm::pair32_sum(fpm::pair16_sum(s));
                    }
                    const int j = wn * 128 + fn * 16 + fr;
                    if (fq == 0) {
                        cm[wm * WN + j] = m;
                        cs[wm * WN + j] = s;
                    }
                    dj[fn] = nd > 0 && j < C ? D[j] : -INFINITY;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __syncthreads();
            if (live) {   // ... then the four row waves' partials, in wave order, and the dummy rows' term
                const Pos p = fresh_pos();
                const int fr = p.fr, fq = p.fq;
#pragma unroll
                for (int fn = 0; fn < FN; ++fn) {
                    const int j = wn * 128 + fn * 16 + fr;
                    const float m0 = cm[j], m1 = cm[WN + j], m2 = cm[2 * WN + j], m3 = cm[3 * WN + j];
                    const float mm = fmaxf(fmaxf(fmaxf(m0, m1), fmaxf(m2, m3)), dj[fn]);
                    const float mf = finite_max(mm);
                    float t = cs[j] * fpm::fast_exp2(m0 - mf);
                    t += cs[WN + j] * fpm::fast_exp2(m1 - mf);
                    t += cs[2 * WN + j] * fpm::fast_exp2(m2 - mf);
                    t += cs[3 * WN + j] * fpm::fast_exp2(m3 - mf);
                    t += fnd * fpm::fast_exp2(dj[fn] - mf);
                    const float lse = mm == -INFINITY ? 0.f : mm + fpm::fast_log2(t);
#pragma unroll
                    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
                        for (int r = 0; r < 4; ++r) L[fm][fn][r] -= lse;
                    if (nd > 0 && wm == 0 && fq == 0 && j < C) D[j] = dj[fn] - lse;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __syncthreads();                         // D and the partials before the next rows step
        }

        {   // <P, Kp> over this thread's accumulator positions, then the wave, then the eight waves
            const Pos p = fresh_pos();
            const int tid = p.tid, lane = p.lane;
            float part = 0.f;
            if (live) {
#pragma unroll
                for (int fm = 0; fm < FM; ++fm) {
#pragma unroll
                    for (int fn = 0; fn < FN; ++fn) {
                        const f32x4_t kp4 = slot[(fm * FN + fn) * WT + tid];
#pragma unroll
                        for (int r = 0; r < 4; ++r) part += fpm::fast_exp2(L[fm][fn][r]) * kp4[r];
                    }
                    __builtin_amdgcn_sched_barrier(0);           // 8 loads in flight
                }
            }
            part = fpm::wave_sum_dpp(part);
            if (lane == 0) red[wave] = part;
            __syncthreads();
            if (tid == 0) {
                float t = red[0];
#pragma unroll
                for (int w = 1; w < WT / 64; ++w) t += red[w];
                score[b] = t / (float)R;
            }
        }
        __syncthreads();                             // red and the tiles before the next pair
    }
}
}  // namespace

extern "C" long fpm_coarse_score_wide_ws_bytes(int B) {
    if (B <= 0) return 0;
    return (long)(B < WGRID ? B : WGRID) * SLOT_FLOATS * (long)sizeof(float);
}

namespace {
// the traits of fpm::coarse_score_entry / coarse_pairs_entry (coarse_probe.h); one slot per workgroup
struct Wide {
    static constexpr const char *score_op = "coarse_score_wide", *pairs_op = "coarse_pairs_wide",
                                *bound = "COARSE_WIDE_NMAX";
    static constexpr int nmax = FPM_COARSE_WIDE_NMAX;
    template <typename YT, bool PAIRS>
    static int launch(const char* what, typename EntryRows<YT>::host y, const long* row_off, const int* idx, int G,
                      int B, const float* ypq, int n0q, const long* qrow_off, const int* qidx, int n0max, const float* coef, int iters, float tau,
                      float* score, void* ws, long ws_bytes, void* stream) {
        const long need = fpm_coarse_score_wide_ws_bytes(B);
        FPM_CHECK_ARG(ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0,
                      "coarse_score_wide: workspace of %ld bytes (16-byte aligned) required, got %ld", need, ws_bytes);
        if (hipFuncSetAttribute((const void*)coarse_score_wide_kernel<YT, PAIRS>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, WLDS) != hipSuccess) {
            (void)hipGetLastError();
            fpm::set_error("coarse_score_wide: %d bytes of LDS per workgroup refused", WLDS);
            return 1;
        }
        const int grid = B < WGRID ? B : WGRID;
        hipLaunchKernelGGL((coarse_score_wide_kernel<YT, PAIRS>), dim3((unsigned)grid), dim3(WT), WLDS,
                           (hipStream_t)stream, y, row_off, idx, G, B, ypq, n0q, coef, iters, tau, score, (float*)ws,
                           qrow_off, qidx);
        return fpm::check_launch(what);
    }
};
}  // namespace

extern "C" int fpm_coarse_score_wide(const float* y, const long* row_off, const int* idx, int G, int B,
                                     const float* yp, int n0, const float* coef, int iters, float tau, float* score,
                                     void* ws, long ws_bytes, void* stream) {
    return fpm::coarse_score_entry<Wide, float>("fpm_coarse_score_wide", y, row_off, idx, G, B, yp, n0, coef, iters, tau, score,
                                         ws, ws_bytes, stream);
}

extern "C" int fpm_coarse_score_wide_rows16(const void* y16, const long* row_off, const int* idx, int G, int B,
                                            const float* yp, int n0, const float* coef, int iters, float tau,
                                            float* score, void* ws, long ws_bytes, void* stream) {
    return fpm::coarse_score_entry<Wide, bf16_t>("fpm_coarse_score_wide_rows16", (const bf16_t*)y16, row_off, idx, G, B, yp, n0,
                                         coef, iters, tau, score, ws, ws_bytes, stream);
}

extern "C" int fpm_coarse_pairs_wide(const float* y, const long* row_off, const int* idx, int G, int B, const float* yq,
                                     const long* qrow_off, const int* qidx, int Q, const float* coef, int iters,
                                     float tau, float* score, void* ws, long ws_bytes, void* stream) {
    return fpm::coarse_pairs_entry<Wide, float>("fpm_coarse_pairs_wide", y, row_off, idx, G, B, yq, qrow_off, qidx, Q, coef,
                                         iters, tau, score, ws, ws_bytes, stream);
}

extern "C" int fpm_coarse_pairs_wide_rows16(const void* y16, const long* row_off, const int* idx, int G, int B,
                                            const float* yq, const long* qrow_off, const int* qidx, int Q,
                                            const float* coef, int iters, float tau, float* score, void* ws,
                                            long ws_bytes, void* stream) {
    return fpm::coarse_pairs_entry<Wide, bf16_t>("fpm_coarse_pairs_wide_rows16", (const bf16_t*)y16, row_off, idx, G, B, yq,
                                         qrow_off, qidx, Q, coef, iters, tau, score, ws, ws_bytes, stream);
}

extern "C" int fpm_coarse_score_wide_rows8(const void* y8, const float* s8, const long* row_off, const int* idx, int G,
                                           int B, const float* yp, int n0, const float* coef, int iters, float tau,
                                           float* score, void* ws, long ws_bytes, void* stream) {
    return fpm::coarse_score_entry<Wide, fp8_t>("fpm_coarse_score_wide_rows8", rows8_t{(const unsigned char*)y8, s8},
                                                row_off, idx, G, B, yp, n0, coef, iters, tau, score, ws, ws_bytes,
                                                stream);
}

extern "C" int fpm_coarse_pairs_wide_rows8(const void* y8, const float* s8, const long* row_off, const int* idx, int G,
                                           int B, const float* yq, const long* qrow_off, const int* qidx, int Q,
                                           const float* coef, int iters, float tau, float* score, void* ws,
                                           long ws_bytes, void* stream) {
    return fpm::coarse_pairs_entry<Wide, fp8_t>("fpm_coarse_pairs_wide_rows8", rows8_t{(const unsigned char*)y8, s8},
                                                row_off, idx, G, B, yq, qrow_off, qidx, Q, coef, iters, tau, score, ws,
                                                ws_bytes, stream);
}

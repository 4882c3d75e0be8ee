// Coarse 1:N score of a probe against enrolled gallery entries (the first pass of a shortlisted
// identification): per (probe, entry) pair one scalar,
//
//     score = sum_{i < n0, j < n_g} P_ij Kp_ij / min(n0, n_g),
//     Kp = softplus(a b^T) - 0.5,  a = bf16(y_p o c),  b = bf16(y_g),
//     P  = Sinkhorn(Kp; dummy rows, iters, tau)          (pygmtools' log-domain Sinkhorn),
//
// the entropy-relaxed assignment value of the vertex affinity per matched keypoint.
//
// One workgroup (256 threads, 4 waves in a 2 x 2 grid of 64 x 64 quadrants) per pair:
//   1. a b^T on v_mfma_f32_16x16x32_bf16.  The fp32 rows come from global memory (the entry's rows
//      once, the probe's from L2), are scaled (probe side: one fp32 multiply by coef[b]) and rounded
//      to bf16 (RNE) on the way into LDS; K = 768 in 12 tiles of 64, the next tile's global loads in
//      flight under the current tile's MFMAs.
//   2. The epilogue leaves Kp in the accumulators (they stay there to the end) and writes
//      L = Kp / tau, in log2 units (so each exp is one v_exp_f32), into a 128 x 128 fp32 matrix in
//      LDS, in the Sinkhorn's own orientation (rows = the smaller side: the MFMA's A operand is that
//      side), over the operand tiles' space.
//   3. The Sinkhorn runs on L in place, as the reference does (L -= lse along rows / columns in
//      turn): the dominant entries of log P sit near 0, where fp32 is fine-grained (a potential
//      form, L = M - u - v, would cancel values of ~100 at every read).  Rows: 16 lanes per row, DPP
//      trees.  Columns: two threads per column, the half column in registers between its one read
//      and its one write.  The nd = C - R dummy rows are identical at every step, so one row (index
//      128) with multiplicity nd stands for them.
//   4. sum exp2(L) Kp over each thread's accumulator positions, wave sums (DPP), the four waves
//      through LDS; 4 bytes out.
// An index that keeps a bf16 copy of its rows (the same RNE rounding, done once at enrolment) hands
// that to the kernel's bf16 instantiation (fpm_coarse_score_rows16): the entry's tile is then copied
// to the same LDS layout in 16-B vectors of 8 bf16, no multiply and no convert, half the bytes
// fetched; the probe side and everything after the tile store are the same code, so are the bits.
// The n0 x n_g block never reaches HBM.  Every order of summation is fixed by the pair alone (K
// order of the MFMA chain, 16-lane DPP trees, the two row halves of a column, the accumulator walk),
// so an entry's score is bit-identical whatever else shares the launch.  No spinning, no exchange
// between workgroups.  LDS: 68.6 KB per workgroup, two workgroups per CU.
#include "fpm_common.h"
#include "coarse_probe.h"
#include "coarse_tile.h"
#include "fpm.h"

namespace {
constexpr int CN = FPM_COARSE_NMAX;      // 128
constexpr int CT = 256;                  // threads
constexpr int CK = 768;                  // channels
constexpr int CBK = 64;                  // K tile
constexpr int CROW = 144;                // bytes per operand row in LDS: 64 bf16 + 16 B pad
constexpr int CTILE = CN * CROW;         // one operand tile
constexpr int SLD = CN + 1;              // fp32 row stride of L (odd: column walks spread over the banks)
constexpr int S_FLOATS = (CN + 1) * SLD; // rows 0..127 and the dummy row 128
constexpr int LDS_FLOATS = S_FLOATS + 4 * CN + 4;
static_assert(2 * CTILE <= S_FLOATS * 4, "the operand tiles share L's space");

using namespace fpm::coarse;
// a K tile: 8 float4 (128 rows) or 4 vectors of 8 bf16 per thread (coarse_tile.h)
using KTile = Tile<CT, CBK, CROW>;

// YT: the entry rows' type, float (rounded on the way into LDS), bf16_t (rounded at enrolment) or fp8_t
// (e4m3 with a row scale, quantised at enrolment and dequantised, exactly, on the way into LDS).
// PAIRS: the probe of pair b comes from a second row store (a pair list: coarse_probe.h); the lookup
// below is the only code that differs.
// two workgroups per CU (LDS allows it): hold the registers to two waves per SIMD
template <typename YT, bool PAIRS>
__global__ __launch_bounds__(CT) __attribute__((amdgpu_waves_per_eu(2, 2))) void coarse_score_kernel(
                                                           typename EntryRows<YT>::arg y,
                                                           const long* __restrict__ row_off,
                                                           const int* __restrict__ idx, int G,
                                                           const float* __restrict__ yp, int n0,
                                                           const float* __restrict__ coef, int iters, float tau,
                                                           float* __restrict__ score,
                                                           const long* __restrict__ qrow_off,
                                                           const int* __restrict__ qidx) {
    extern __shared__ float lds[];
    float* S = lds;
    float* cm = lds + S_FLOATS;              // [2][128] column partial maxima
    float* cs = cm + 2 * CN;                 // [2][128] column partial sums
    float* red = cs + 2 * CN;                // [4] wave sums
    unsigned char* At = (unsigned char*)lds; // operand tiles (before L exists)
    unsigned char* Bt = At + CTILE;

    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = idx[b];
    long r0 = 0, ngl = 0;
    if (g >= 0 && g < G) {
        r0 = row_off[g];
        ngl = row_off[g + 1] - r0;
    }
    if constexpr (PAIRS) {                   // a pair list: yp is the probe row store and n0 its graph count
        const float* yb;
        int nb;
        fpm::coarse_probe_of<true>(yp, n0, qrow_off, qidx, b, yb, nb);
        yp = yb;
        n0 = nb;
    }
    // the wrapper checks both on the host; never read outside y, never index past the 128 x 128 box
    if (ngl < 1 || ngl > CN || n0 < 1 || n0 > CN) {
        if (tid == 0) score[b] = __uint_as_float(0x7FC00000u);
        return;
    }
    const int ng = (int)ngl;
    // the Sinkhorn works on the transpose when n0 > n_g: its rows are the smaller side
    const bool tr = n0 > ng;
    const int R = tr ? ng : n0, C = tr ? n0 : ng;
    constexpr bool F32 = sizeof(YT) == 4, F8 = sizeof(YT) == 1;
    const auto ye = y + r0 * CK;                   // the entry's rows
    const float* xa = nullptr;                       // rows side (MFMA A)
    const float* xb = nullptr;                       // columns side (MFMA B)
    if constexpr (F32) {
        xa = tr ? ye : yp;
        xb = tr ? yp : ye;
    }
    // bf16 and fp8 entry rows: the probe's tile is At and the entry's Bt, the other way round when transposed
    unsigned char* Pt = tr ? Bt : At;
    unsigned char* Et = tr ? At : Bt;
    const float* cf = coef + (long)b * CK;
    const int c4 = 4 * (tid & 15);
    const float4 one = make_float4(1.f, 1.f, 1.f, 1.f);

    const int wm = wave >> 1, wn = wave & 1;
    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    float4 ra[8], rb[8], sc;
    uint4 re[4];
    uint2 r8[4];
    float s8[4];
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
    const int fr = lane & 15, fq = lane >> 4;
    for (int kt = 0; kt < CK / CBK; ++kt) {
        if constexpr (F32) {
            KTile::store(At, tid, ra, tr ? one : sc);
            KTile::store(Bt, tid, rb, tr ? sc : one);
        } else if constexpr (F8) {
            KTile::store(Pt, tid, ra, sc);
            KTile::store8(Et, tid, r8, s8);
        } else {
            KTile::store(Pt, tid, ra, sc);
            KTile::store16(Et, tid, re);
        }
        __syncthreads();
        if (kt + 1 < CK / CBK) {
            if constexpr (F32) {
                KTile::load(xa, R, 0, (kt + 1) * CBK, tid, ra);
                KTile::load(xb, C, 0, (kt + 1) * CBK, tid, rb);
            } else if constexpr (F8) {
                KTile::load(yp, n0, 0, (kt + 1) * CBK, tid, ra);
                KTile::load8(ye, ng, 0, (kt + 1) * CBK, tid, r8);
            } else {
                KTile::load(yp, n0, 0, (kt + 1) * CBK, tid, ra);
                KTile::load16(ye, ng, 0, (kt + 1) * CBK, tid, re);
            }
            sc = *(const float4*)(cf + (kt + 1) * CBK + c4);
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8_t a[4], bb[4];
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                a[f] = *(const bf16x8_t*)(At + (wm * 64 + f * 16 + fr) * CROW + (kk * 32 + fq * 8) * 2);
                bb[f] = *(const bf16x8_t*)(Bt + (wn * 64 + f * 16 + fr) * CROW + (kk * 32 + fq * 8) * 2);
            }
#pragma unroll
            for (int fm = 0; fm < 4; ++fm) {
                if (wm * 64 + fm * 16 >= R) continue;        // fragments past the block: wave-uniform
#pragma unroll
                for (int fn = 0; fn < 4; ++fn) {
                    if (wn * 64 + fn * 16 >= C) continue;
                    acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[fm], bb[fn], acc[fm][fn], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // Kp stays in acc (0 outside the block); L = Kp / tau into LDS
#pragma unroll
    for (int fm = 0; fm < 4; ++fm)
#pragma unroll
        for (int fn = 0; fn < 4; ++fn)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = wm * 64 + fm * 16 + 4 * fq + r, j = wn * 64 + fn * 16 + fr;
                float kp = 0.f;
                if (i < R && j < C) {
                    kp = fpm::softplus_f(acc[fm][fn][r]) - 0.5f;
                    S[i * SLD + j] = (kp / tau) * fpm::LOG2E_F;
                }
                acc[fm][fn][r] = kp;
            }
    const int nd = C - R;                    // dummy rows (dummy_row = True)
    if (nd > 0 && tid < C) S[CN * SLD + tid] = -100.f * fpm::LOG2E_F;
    __syncthreads();

    const float fnd = (float)nd;
    for (int it = 0; it < iters; ++it) {
        if ((it & 1) == 0) {
            // rows: 16 lanes per row, 8 columns per lane.  A wave's four rows lie 16 apart (row stride
            // 129 words: 16 banks apart, no conflicts); pass 8 is the dummy row's
            for (int u = 0; u < 9; ++u) {
                const int p = u < 8 ? (u >> 2) * 64 + fq * 16 + wave * 4 + (u & 3) : (wave == 0 && fq == 0 ? CN : -1);
                if (p < 0 || (p < CN ? p >= R : nd <= 0)) continue;
                float* row = S + p * SLD;
                float x[8];
                float m = -INFINITY;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int c = fr + 16 * q;
                    x[q] = c < C ? row[c] : -INFINITY;
                    m = fmaxf(m, x[q]);
                }
                m = row16_max(m);
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < 8; ++q) s += fpm::fast_exp2(x[q] - m);
                s = fpm::row16_sum(s);
                const float lse = m + fpm::fast_log2(s);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int c = fr + 16 * q;
                    if (c < C) row[c] = x[q] - lse;
                }
            }
        } else {
            // columns: two threads per column, rows [0, 64) and [64, 128); the first also takes the
            // nd dummy rows; the halves join through LDS in a fixed order
            const int j = tid & (CN - 1), h = tid >> 7;
            const int i0 = h * 64, i1 = R < i0 + 64 ? R : i0 + 64;
            const bool dm = nd > 0 && h == 0;
            // the half column in two chunks of 32 rows (32 independent loads in flight each); their
            // (max, sum) pairs merge in a fixed order, then the dummy rows' term
            float m = -INFINITY, s = 0.f, dj = 0.f;
            const bool on = j < C;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int ib = i0 + 32 * c;
                if (!on || ib >= i1) continue;
                float x[32];
                float mc = -INFINITY, sc2 = 0.f;
#pragma unroll
                for (int q = 0; q < 32; ++q) {
                    x[q] = ib + q < i1 ? S[(ib + q) * SLD + j] : -INFINITY;
                    mc = fmaxf(mc, x[q]);
                }
#pragma unroll
                for (int q = 0; q < 32; ++q) sc2 += fpm::fast_exp2(x[q] - mc);
                if (c == 0) {
                    m = mc;
                    s = sc2;
                } else {
                    const float mn = fmaxf(m, mc);
                    s = s * fpm::fast_exp2(m - mn) + sc2 * fpm::fast_exp2(mc - mn);
                    m = mn;
                }
            }
            if (on) {
                if (dm) {                                        // half 0: never empty (row 0)
                    dj = S[CN * SLD + j];
                    const float mn = fmaxf(m, dj);
                    s = s * fpm::fast_exp2(m - mn) + fnd * fpm::fast_exp2(dj - mn);
                    m = mn;
                }
                cm[h * CN + j] = m;                              // (-inf, 0): an empty half 1
                cs[h * CN + j] = s;
            }
            __syncthreads();
            if (on) {
                const float m0 = cm[j], m1 = cm[CN + j];
                const float mm = fmaxf(m0, m1);              // finite: half 0 holds row 0
                const float t = cs[j] * fpm::fast_exp2(m0 - mm) + cs[CN + j] * fpm::fast_exp2(m1 - mm);
                const float lse = mm + fpm::fast_log2(t);
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int ib = i0 + 32 * c;
                    if (ib >= i1) continue;
                    float x[32];
#pragma unroll
                    for (int q = 0; q < 32; ++q) x[q] = ib + q < i1 ? S[(ib + q) * SLD + j] : 0.f;
#pragma unroll
                    for (int q = 0; q < 32; ++q)
                        if (ib + q < i1) S[(ib + q) * SLD + j] = x[q] - lse;
                }
                if (dm) S[CN * SLD + j] = dj - lse;
            }
        }
        __syncthreads();
    }

    // <P, Kp> over this thread's accumulator positions, then the wave, then the four waves
    float part = 0.f;
#pragma unroll
    for (int fm = 0; fm < 4; ++fm)
#pragma unroll
        for (int fn = 0; fn < 4; ++fn)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = wm * 64 + fm * 16 + 4 * fq + r, j = wn * 64 + fn * 16 + fr;
                if (i < R && j < C) part += fpm::fast_exp2(S[i * SLD + j]) * acc[fm][fn][r];
            }
    part = fpm::wave_sum_dpp(part);
    if (lane == 0) red[wave] = part;
    __syncthreads();
    if (tid == 0) score[b] = (((red[0] + red[1]) + red[2]) + red[3]) / (float)R;
}
}  // namespace

namespace {
// the traits of fpm::coarse_score_entry / coarse_pairs_entry (coarse_probe.h); no workspace
struct Fused {
    static constexpr const char *score_op = "coarse_score", *pairs_op = "coarse_pairs", *bound = "COARSE_NMAX";
    static constexpr int nmax = FPM_COARSE_NMAX;
    template <typename YT, bool PAIRS>
    static int launch(const char* what, typename EntryRows<YT>::host y, const long* row_off, const int* idx, int G,
                      int B, const float* ypq, int n0q, const long* qrow_off, const int* qidx, int n0max, const float* coef, int iters, float tau,
                      float* score, void* ws, long ws_bytes, void* stream) {
        constexpr int lds = LDS_FLOATS * (int)sizeof(float);
        if (hipFuncSetAttribute((const void*)coarse_score_kernel<YT, PAIRS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                lds) != hipSuccess) {
            (void)hipGetLastError();
            fpm::set_error("coarse_score: %d bytes of LDS per workgroup refused", lds);
            return 1;
        }
        hipLaunchKernelGGL((coarse_score_kernel<YT, PAIRS>), dim3((unsigned)B), dim3(CT), lds, (hipStream_t)stream, y,
                           row_off, idx, G, ypq, n0q, coef, iters, tau, score, qrow_off, qidx);
        return fpm::check_launch(what);
    }
};
}  // namespace

extern "C" int fpm_coarse_score(const float* y, const long* row_off, const int* idx, int G, int B, const float* yp,
                                int n0, const float* coef, int iters, float tau, float* score, void* stream) {
    return fpm::coarse_score_entry<Fused, float>("fpm_coarse_score", y, row_off, idx, G, B, yp, n0, coef, iters, tau, score,
                                          nullptr, 0, stream);
}

extern "C" int fpm_coarse_score_rows16(const void* y16, const long* row_off, const int* idx, int G, int B,
                                       const float* yp, int n0, const float* coef, int iters, float tau, float* score,
                                       void* stream) {
    return fpm::coarse_score_entry<Fused, bf16_t>("fpm_coarse_score_rows16", (const bf16_t*)y16, row_off, idx, G, B, yp, n0,
                                          coef, iters, tau, score, nullptr, 0, stream);
}

extern "C" int fpm_coarse_pairs(const float* y, const long* row_off, const int* idx, int G, int B, const float* yq,
                                const long* qrow_off, const int* qidx, int Q, const float* coef, int iters, float tau,
                                float* score, void* stream) {
    return fpm::coarse_pairs_entry<Fused, float>("fpm_coarse_pairs", y, row_off, idx, G, B, yq, qrow_off, qidx, Q, coef, iters,
                                          tau, score, nullptr, 0, stream);
}

extern "C" int fpm_coarse_pairs_rows16(const void* y16, const long* row_off, const int* idx, int G, int B,
                                       const float* yq, const long* qrow_off, const int* qidx, int Q, const float* coef,
                                       int iters, float tau, float* score, void* stream) {
    return fpm::coarse_pairs_entry<Fused, bf16_t>("fpm_coarse_pairs_rows16", (const bf16_t*)y16, row_off, idx, G, B, yq,
                                          qrow_off, qidx, Q, coef, iters, tau, score, nullptr, 0, stream);
}

extern "C" int fpm_coarse_score_rows8(const void* y8, const float* s8, const long* row_off, const int* idx, int G, int B,
                                      const float* yp, int n0, const float* coef, int iters, float tau, float* score,
                                      void* stream) {
    return fpm::coarse_score_entry<Fused, fp8_t>("fpm_coarse_score_rows8", rows8_t{(const unsigned char*)y8, s8},
                                                 row_off, idx, G, B, yp, n0, coef, iters, tau, score, nullptr, 0,
                                                 stream);
}

extern "C" int fpm_coarse_pairs_rows8(const void* y8, const float* s8, const long* row_off, const int* idx, int G, int B,
                                      const float* yq, const long* qrow_off, const int* qidx, int Q, const float* coef,
                                      int iters, float tau, float* score, void* stream) {
    return fpm::coarse_pairs_entry<Fused, fp8_t>("fpm_coarse_pairs_rows8", rows8_t{(const unsigned char*)y8, s8},
                                                 row_off, idx, G, B, yq, qrow_off, qidx, Q, coef, iters, tau, score,
                                                 nullptr, 0, stream);
}

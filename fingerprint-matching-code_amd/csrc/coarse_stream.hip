// The coarse 1:N score of coarse.hip (same definition, see there) for boxes of up to 600 keypoints
// (FPM_COARSE_STREAM_NMAX = the matcher's own cap):
//
//     score = sum_{i < n0, j < n_g} P_ij Kp_ij / min(n0, n_g),
//     Kp = softplus(a b^T) - 0.5,  a = bf16(y_p o c),  b = bf16(y_g),
//     P  = Sinkhorn(Kp; dummy rows, iters, tau)          (pygmtools' log-domain Sinkhorn).
//
// A 600 x 600 fp32 block is 1.44 MB: it fits neither the LDS (coarse.hip) nor the registers
// (coarse_wide.hip) of a CU, so it lives in the workgroup's own slot of a device workspace and is
// streamed from L2 / Infinity Cache.  One workgroup of 512 threads per pair, R = the smaller side
// as the Sinkhorn's rows, C the larger, the slot row-major R x C4 (C4 = C rounded up to 4):
//   1. Kp, tile by tile: 128 entry rows (MFMA A) x 256 probe rows (MFMA B) whichever side is R, so
//      the entry's rows, which no other workgroup shares, are read ceil(n0 / 256) times and the
//      probe's, hot in L2 for the whole launch, ceil(n_g / 128) times; 8 waves in a 2 x 4 grid, a
//      wave's 64 x 64 part in 4 x 4 fragments of v_mfma_f32_16x16x32_bf16.  The fp32 operand rows
//      come from global memory, are scaled (probe side: one fp32 multiply) and rounded to bf16 on
//      the way into LDS; K = 768 in 12 tiles of 64, two LDS buffers, one barrier per K tile, the
//      next K tile's loads in flight under the MFMAs.  Rows past n_g / n0 are zero-filled without
//      being read.  The epilogue writes Kp = softplus - 0.5 in fp32 at its place in the R x C4 slot
//      (0 in the columns [C, C4)); nothing else of the slot is ever read, so the workspace needs
//      no clearing.
//   2. The Sinkhorn, in log2 units.  The first row step is taken in place: L1 = L0 - rowlse(L0),
//      L0 = Kp log2(e) / tau; only the row's lse r1_i is kept, and L1_ij = fl(fl(Kp_ij s) - r1_i) is
//      rebuilt, the same bits, wherever it is read.  The remaining iters - 1 steps run on potentials
//      over L1: L = (L1 - u_i) - v_j, u and v in LDS, each step adding the line's lse to its
//      potential.  (Potentials over L0 itself reach ~100 / tau-scaled magnitudes and every read
//      rounds at their ulp: that form misses the float64 gate)  A row step: one wave
//      per row, four rows in flight, lanes along the row in 16-B loads, the row's max and sum on the
//      wave (DPP).  A column step: a thread owns four adjacent columns over the rows rg, rg + nrg,
//      ... (online max-rescaled sums, eight rows in flight), the nrg row groups' (max, sum) partials
//      through LDS, merged in group order, then the dummy rows' term.  The nd = C - R identical
//      dummy rows are one vector of multiplicity nd in LDS, updated in place.
//   3. sum exp2(L) Kp in the column step's walk, the wave (DPP), the eight waves in wave order.
// The grid is persistent: min(B, 256) workgroups, workgroup w takes pairs w, w + grid, ...; one slot
// per workgroup.  The block passes between the threads of one workgroup only (a barrier after the
// stores); no exchange between workgroups, no spinning, no atomics.  Every order of summation is
// fixed by (R, C) alone, so a score is the same bits whatever shares the launch, whichever
// workgroup computes it and however large the slots are.  LDS: 134.0 KB per workgroup.
#include "fpm_common.h"
#include "coarse_probe.h"
#include "coarse_tile.h"
#include "fpm.h"

namespace {
constexpr int SN = FPM_COARSE_STREAM_NMAX;   // 600
constexpr int SP = 640;                      // a potential vector in LDS
constexpr int ST = 512;                      // threads
constexpr int SK = 768;                      // channels
constexpr int SBK = 64;                      // K tile: two MFMA steps of 32
constexpr int SROW = 144;                    // bytes per operand row in LDS: 64 bf16 + 16 B pad
constexpr int TM = 128, TN = 256;            // a block tile
constexpr int ATILE = TM * SROW, BTILE = TN * SROW, SBUF = ATILE + BTILE;
constexpr int SGRID = 256;                   // workgroups at most (one per CU)
constexpr int FM = 4, FN = 4;                // a wave's fragments: 64 rows x 64 columns
constexpr int PART = 4 * ST;                 // column partials: nrg x C4 <= 2048
// LDS after the two tile buffers: r1, u, v, D, the column partials (max, sum), the wave sums
constexpr int RED_FLOATS = 4 * SP + 2 * PART + 8;
constexpr int SLDS = 2 * SBUF + RED_FLOATS * 4;
constexpr int RW = 4;                        // rows in flight per wave in a row step
constexpr int CU = 8;                        // rows in flight per thread in a column step

using namespace fpm::coarse;
// a K tile: 4 (entry, 128 rows) or 8 (probe, 256 rows) float4, or 2 vectors of 8 bf16, per thread
// (coarse_tile.h)
using KTile = Tile<ST, SBK, SROW>;

// L_ij from Kp_ij: every rounding spelled out (no contraction), so every reader rebuilds the same
// bits: L1 = fl(fl(Kp s) - r1) is the in-place first step's value, then the two potentials
__device__ __forceinline__ float lval(float kp, float s, float r1, float u, float v) {
    return __fsub_rn(__fsub_rn(__fsub_rn(__fmul_rn(kp, s), r1), u), v);
}

// YT: the entry rows' type, float (rounded on the way into LDS), bf16_t (rounded at enrolment) or fp8_t
// (e4m3 with a row scale, quantised at enrolment and dequantised, exactly, on the way into LDS); the
// probe side and everything after the tile store are the same code, so are the bits.  PAIRS: the probe
// of pair b comes from a second row store (a pair list: coarse_probe.h), looked up per pair of the
// persistent walk; that lookup is the only code that differs
template <typename YT, bool PAIRS>
__global__ __launch_bounds__(ST) void coarse_score_stream_kernel(typename EntryRows<YT>::arg y,
                                                                 const long* __restrict__ row_off,
                                                                 const int* __restrict__ idx, int G, int B,
                                                                 const float* __restrict__ ypq, int n0q,
                                                                 const float* __restrict__ coef, int iters, float tau,
                                                                 float* __restrict__ score, float* ws,
                                                                 long slot_floats, const long* __restrict__ qrow_off,
                                                                 const int* __restrict__ qidx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char slds[];
    float* r1 = (float*)(slds + 2 * SBUF);   // [640] the first row step's lse
    float* u = r1 + SP;                      // [640] row potentials
    float* v = u + SP;                       // [640] column potentials
    float* D = v + SP;                       // [640] the dummy rows' vector
    float* pm = D + SP;                      // [nrg][C4] column partial maxima
    float* ps = pm + PART;                   // [nrg][C4] column partial sums
    float* red = ps + PART;                  // [8] wave sums

    const int tid = threadIdx.x, lane = tid & 63, fr = tid & 15, fq = (tid >> 4) & 3;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar: wave-uniform branches
    const int wm = wave >> 2, wn = wave & 3;
    float* slot = ws + (long)blockIdx.x * slot_floats;
    const float sc = fpm::LOG2E_F / tau;

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
        // the wrapper checks both on the host; never read outside y, never index past the slot
        bool bad = ngl < 1 || ngl > SN || n0 < 1 || n0 > SN;
        const int ng = bad ? 1 : (int)ngl;
        // the Sinkhorn works on the transpose when n0 > n_g: its rows are the smaller side
        const bool tr = n0 > ng;
        const int R = tr ? ng : n0, C = tr ? n0 : ng;
        const int C4 = (C + 3) & ~3;
        bad = bad || (long)R * C4 > slot_floats;
        if (bad) {                                   // uniform over the workgroup
            if (tid == 0) score[b] = __uint_as_float(0x7FC00000u);
            continue;
        }
        constexpr bool F32 = sizeof(YT) == 4, F8 = sizeof(YT) == 1;
        const auto xe = y + r0 * SK;               // the entry's rows: MFMA A, tiles of 128
        const float* cf = coef + (long)b * SK;
        const int nd = C - R;                        // dummy rows (dummy_row = True)
        const float fnd = (float)nd;

        // ---- 1. Kp into the slot, tile by tile: entry rows e x probe rows p, whichever side is R
        for (int te = 0; te < ng; te += TM)
            for (int tp = 0; tp < n0; tp += TN) {
                f32x4_t acc[FM][FN];
#pragma unroll
                for (int i = 0; i < FM; ++i)
#pragma unroll
                    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
                const int c4 = 4 * (tid & 15);
                const float4 one = make_float4(1.f, 1.f, 1.f, 1.f);
                float4 ra[4], rb[8], s4;
                uint4 re[2];                             // bf16 entry rows, in ra's place
                uint2 r8[2];                             // fp8 entry rows and their rows' scales, in ra's place
                float s8[2];
                if constexpr (F32) KTile::load(xe, ng, te, 0, tid, ra);
                else if constexpr (F8) {
                    KTile::load8(xe, ng, te, 0, tid, r8);
                    KTile::load8_scale(xe, ng, te, tid, s8);
                } else KTile::load16(xe, ng, te, 0, tid, re);
                KTile::load(yp, n0, tp, 0, tid, rb);
                s4 = *(const float4*)(cf + c4);
                for (int kt = 0; kt < SK / SBK; ++kt) {
                    unsigned char* At = slds + (kt & 1) * SBUF;
                    unsigned char* Bt = At + ATILE;
                    if constexpr (F32) KTile::store(At, tid, ra, one);
                    else if constexpr (F8) KTile::store8(At, tid, r8, s8);
                    else KTile::store16(At, tid, re);
                    KTile::store(Bt, tid, rb, s4);
                    // one barrier per K tile: the other buffer was last read before the previous barrier
                    // (12 K tiles, an even count: the parity carries over from one block tile to the next)
                    __syncthreads();
                    if (kt + 1 < SK / SBK) {
                        if constexpr (F32) KTile::load(xe, ng, te, (kt + 1) * SBK, tid, ra);
                        else if constexpr (F8) KTile::load8(xe, ng, te, (kt + 1) * SBK, tid, r8);
                        else KTile::load16(xe, ng, te, (kt + 1) * SBK, tid, re);
                        KTile::load(yp, n0, tp, (kt + 1) * SBK, tid, rb);
                        s4 = *(const float4*)(cf + (kt + 1) * SBK + c4);
                    }
#pragma unroll
                    for (int kk = 0; kk < SBK / 32; ++kk) {
                        bf16x8_t a[FM];
#pragma unroll
                        for (int f = 0; f < FM; ++f)
                            a[f] = *(const bf16x8_t*)(At + (wm * 64 + f * 16 + fr) * SROW + kk * 64 + fq * 16);
#pragma unroll
                        for (int fn = 0; fn < FN; ++fn) {
                            if (tp + wn * 64 + fn * 16 >= n0) continue;  // fragments past the block: wave-uniform
                            const bf16x8_t bb =
                                *(const bf16x8_t*)(Bt + (wn * 64 + fn * 16 + fr) * SROW + kk * 64 + fq * 16);
#pragma unroll
                            for (int fm = 0; fm < FM; ++fm) {
                                if (te + wm * 64 + fm * 16 >= ng) continue;
                                acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[fm], bb, acc[fm][fn], 0, 0, 0);
                            }
                        }
                    }
                }
                // accumulator r of a fragment: entry row e0 + r (e0 = .. + 4 fq), probe row p (.. + fr)
#pragma unroll
                for (int fm = 0; fm < FM; ++fm)
#pragma unroll
                    for (int fn = 0; fn < FN; ++fn) {
                        // fragments wholly past the block and its padding columns: wave-uniform
                        if (te + wm * 64 + fm * 16 >= ((ng + 3) & ~3) || tp + wn * 64 + fn * 16 >= ((n0 + 3) & ~3)) continue;
                        const int e0 = te + wm * 64 + fm * 16 + 4 * fq, p = tp + wn * 64 + fn * 16 + fr;
                        float kp[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) kp[r] = softplus_native(acc[fm][fn][r]) - 0.5f;
                        if (tr) {                    // rows = the entry's: slot[e][p], 64-B runs along p
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (e0 + r < R && p < C4) slot[(e0 + r) * C4 + p] = p < C ? kp[r] : 0.f;
                        } else if (p < R && e0 < C4) {   // rows = the probe's: slot[p][e0 .. e0 + 3], 16 B
                            *(float4*)(slot + p * C4 + e0) =
                                make_float4(e0 + 0 < C ? kp[0] : 0.f, e0 + 1 < C ? kp[1] : 0.f,
                                            e0 + 2 < C ? kp[2] : 0.f, e0 + 3 < C ? kp[3] : 0.f);
                        }
                    }
            }
        for (int k = tid; k < SP; k += ST) {
            r1[k] = 0.f;
            u[k] = 0.f;
            v[k] = 0.f;
            D[k] = -100.f * fpm::LOG2E_F;
        }
        // the block passes to the workgroup's other threads: stores visible, then the barrier
        __threadfence_block();
        __syncthreads();

        const int nq = C4 >> 2;                                  // 16-B quads per row, <= 150
        // ---- 2a. a row step: u_i += lse_j L_ij (first: r1_i = lse_j L0_ij, with r1 = u = v = 0)
        auto row_step = [&](bool first) {
            if (wave == 0 && nd > 0) {
                // the dummy rows: one row over all C columns
                float m = -INFINITY;
                for (int c = lane; c < C; c += 64) m = fmaxf(m, D[c]);
                m = fpm::warp_max(m);                            // finite: column 0 exists
                float s = 0.f;
                for (int c = lane; c < C; c += 64) s += fpm::fast_exp2(D[c] - m);
                s = fpm::warp_sum(s);
                const float lse = m + fpm::fast_log2(s);
                for (int c = lane; c < C; c += 64) D[c] -= lse;
            }
            float4 vj[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int q = lane + 64 * t;
                vj[t] = q < nq ? *(const float4*)(v + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            for (int i0 = wave * RW; i0 < R; i0 += 8 * RW) {
                float4 x[RW][3];
#pragma unroll
                for (int r = 0; r < RW; ++r)
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        const int q = lane + 64 * t;
                        x[r][t] = (i0 + r < R && q < nq) ? *(const float4*)(slot + (i0 + r) * C4 + 4 * q)
                                                         : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    const int i = i0 + r;
                    if (i >= R) break;                           // wave-uniform
                    const float ri = r1[i], ui = u[i];
                    float m = -INFINITY;
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        const int j = 4 * (lane + 64 * t);
                        x[r][t].x = j + 0 < C ? lval(x[r][t].x, sc, ri, ui, vj[t].x) : -INFINITY;
                        x[r][t].y = j + 1 < C ? lval(x[r][t].y, sc, ri, ui, vj[t].y) : -INFINITY;
                        x[r][t].z = j + 2 < C ? lval(x[r][t].z, sc, ri, ui, vj[t].z) : -INFINITY;
                        x[r][t].w = j + 3 < C ? lval(x[r][t].w, sc, ri, ui, vj[t].w) : -INFINITY;
                        m = fmaxf(fmaxf(m, fmaxf(x[r][t].x, x[r][t].y)), fmaxf(x[r][t].z, x[r][t].w));
                    }
                    m = fpm::warp_max(m);
                    const float mf = finite_max(m);
                    float s = 0.f;
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        s += fpm::fast_exp2(x[r][t].x - mf);
                        s += fpm::fast_exp2(x[r][t].y - mf);
                        s += fpm::fast_exp2(x[r][t].z - mf);
                        s += fpm::fast_exp2(x[r][t].w - mf);
                    }
                    s = fpm::warp_sum(s);
                    const float lse = m == -INFINITY ? 0.f : m + fpm::fast_log2(s);
                    if (lane == 0) {
                        if (first) r1[i] = lse;
                        else u[i] = ui + lse;
                    }
                }
            }
            __syncthreads();
        };

        // the column walk: thread -> quad cq of the row, row group rg; rows rg, rg + nrg, ...
        int nrg = ST / nq;
        nrg = nrg < R ? nrg : R;
        const bool act = tid < nq * nrg;
        const int cq = tid % nq, rg = tid / nq;
        const int j0 = 4 * cq;

        // ---- 2b. a column step: v_j += lse_i L_ij (with the nd dummy rows), D_j -= the same
        auto col_step = [&]() {
            if (act) {
                const float4 vq = *(const float4*)(v + j0);
                float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, s[4] = {0.f, 0.f, 0.f, 0.f};
                for (int i0 = rg; i0 < R; i0 += CU * nrg) {
                    float4 x[CU];
#pragma unroll
                    for (int k = 0; k < CU; ++k) {
                        const int i = i0 + k * nrg;
                        x[k] = i < R ? *(const float4*)(slot + i * C4 + j0) : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                    float bm[4] = {m[0], m[1], m[2], m[3]};
#pragma unroll
                    for (int k = 0; k < CU; ++k) {
                        const int i = i0 + k * nrg;
                        const bool in = i < R;
                        const float ri = in ? r1[i] : 0.f, ui = in ? u[i] : 0.f;
                        x[k].x = in ? lval(x[k].x, sc, ri, ui, vq.x) : -INFINITY;
                        x[k].y = in ? lval(x[k].y, sc, ri, ui, vq.y) : -INFINITY;
                        x[k].z = in ? lval(x[k].z, sc, ri, ui, vq.z) : -INFINITY;
                        x[k].w = in ? lval(x[k].w, sc, ri, ui, vq.w) : -INFINITY;
                        bm[0] = fmaxf(bm[0], x[k].x);
                        bm[1] = fmaxf(bm[1], x[k].y);
                        bm[2] = fmaxf(bm[2], x[k].z);
                        bm[3] = fmaxf(bm[3], x[k].w);
                    }
                    // online: the running sums rescaled once per batch of rows
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        s[c] *= fpm::fast_exp2(m[c] - finite_max(bm[c]));
                        m[c] = bm[c];
                    }
#pragma unroll
                    for (int k = 0; k < CU; ++k) {
                        s[0] += fpm::fast_exp2(x[k].x - finite_max(m[0]));
                        s[1] += fpm::fast_exp2(x[k].y - finite_max(m[1]));
                        s[2] += fpm::fast_exp2(x[k].z - finite_max(m[2]));
                        s[3] += fpm::fast_exp2(x[k].w - finite_max(m[3]));
                    }
                }
                *(float4*)(pm + rg * C4 + j0) = make_float4(m[0], m[1], m[2], m[3]);
                *(float4*)(ps + rg * C4 + j0) = make_float4(s[0], s[1], s[2], s[3]);
            }
            __syncthreads();
            for (int j = tid; j < C; j += ST) {      // the row groups' partials in group order, then the dummy rows
                const float dj = nd > 0 ? D[j] : -INFINITY;
                float mm = dj;
                for (int q = 0; q < nrg; ++q) mm = fmaxf(mm, pm[q * C4 + j]);
                const float mf = finite_max(mm);
                float t = 0.f;
                for (int q = 0; q < nrg; ++q) t += ps[q * C4 + j] * fpm::fast_exp2(pm[q * C4 + j] - mf);
                t += fnd * fpm::fast_exp2(dj - mf);
                const float lse = mm == -INFINITY ? 0.f : mm + fpm::fast_log2(t);
                v[j] += lse;
                if (nd > 0) D[j] = dj - lse;
            }
            __syncthreads();
        };

        int it = 0;
        if (iters > 0) {
            row_step(true);
            it = 1;
        }
        for (; it < iters; ++it) {
            if (it & 1) col_step();
            else row_step(false);
        }

        // ---- 3. <P, Kp> in the column step's walk, then the wave, then the eight waves
        float part = 0.f;
        if (act) {
            const float4 vq = *(const float4*)(v + j0);
            for (int i0 = rg; i0 < R; i0 += CU * nrg) {
                float4 x[CU];
#pragma unroll
                for (int k = 0; k < CU; ++k) {
                    const int i = i0 + k * nrg;
                    x[k] = i < R ? *(const float4*)(slot + i * C4 + j0) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int k = 0; k < CU; ++k) {
                    const int i = i0 + k * nrg;
                    if (i >= R) break;
                    const float ri = r1[i], ui = u[i];
                    if (j0 + 0 < C) part += fpm::fast_exp2(lval(x[k].x, sc, ri, ui, vq.x)) * x[k].x;
                    if (j0 + 1 < C) part += fpm::fast_exp2(lval(x[k].y, sc, ri, ui, vq.y)) * x[k].y;
                    if (j0 + 2 < C) part += fpm::fast_exp2(lval(x[k].z, sc, ri, ui, vq.z)) * x[k].z;
                    if (j0 + 3 < C) part += fpm::fast_exp2(lval(x[k].w, sc, ri, ui, vq.w)) * x[k].w;
                }
            }
        }
        part = fpm::wave_sum_dpp(part);
        if (lane == 0) red[wave] = part;
        __syncthreads();
        if (tid == 0) {
            float t = red[0];
#pragma unroll
            for (int w = 1; w < ST / 64; ++w) t += red[w];
            score[b] = t / (float)R;
        }
        __syncthreads();                             // red, the potentials and the slot before the next pair
    }
}

long slot_floats_of(int n0, int ngmax) {
    const long rm = n0 < ngmax ? n0 : ngmax, cm = n0 < ngmax ? ngmax : n0;
    return rm * ((cm + 3) & ~3L);
}
}  // namespace

extern "C" long fpm_coarse_score_stream_ws_bytes(int B, int n0, int ngmax) {
    if (B <= 0 || n0 < 1 || ngmax < 1) return 0;
    n0 = n0 < SN ? n0 : SN;
    ngmax = ngmax < SN ? ngmax : SN;
    return (long)(B < SGRID ? B : SGRID) * slot_floats_of(n0, ngmax) * (long)sizeof(float);
}

namespace {
// the traits of fpm::coarse_score_entry / coarse_pairs_entry (coarse_probe.h).  The slots are as large as
// the workspace allows; ``need`` is the smallest that serves any pair at all: the largest probe of the
// launch against an entry of one keypoint.  The caller sizes them from the largest probe and the largest
// entry (fpm_coarse_score_stream_ws_bytes(B, n0max, ngmax)); a pair whose block does not fit its slot gets
// NaN
struct Stream {
    static constexpr const char *score_op = "coarse_score_stream", *pairs_op = "coarse_pairs_stream",
                                *bound = "COARSE_STREAM_NMAX";
    static constexpr int nmax = FPM_COARSE_STREAM_NMAX;
    template <typename YT, bool PAIRS>
    static int launch(const char* what, typename EntryRows<YT>::host y, const long* row_off, const int* idx, int G,
                      int B, const float* ypq, int n0q, const long* qrow_off, const int* qidx, int n0max, const float* coef, int iters, float tau,
                      float* score, void* ws, long ws_bytes, void* stream) {
        const int grid = B < SGRID ? B : SGRID;
        const long need = fpm_coarse_score_stream_ws_bytes(B, n0max, 1);
        const long slot_floats = ws_bytes > 0 ? (ws_bytes / (long)sizeof(float) / grid) & ~3L : 0;
        FPM_CHECK_ARG(ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0,
                      "coarse_score_stream: workspace of at least %ld bytes (16-byte aligned; "
                      "fpm_coarse_score_stream_ws_bytes) required, got %ld",
                      need, ws_bytes);
        if (hipFuncSetAttribute((const void*)coarse_score_stream_kernel<YT, PAIRS>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, SLDS) != hipSuccess) {
            (void)hipGetLastError();
            fpm::set_error("coarse_score_stream: %d bytes of LDS per workgroup refused", SLDS);
            return 1;
        }
        hipLaunchKernelGGL((coarse_score_stream_kernel<YT, PAIRS>), dim3((unsigned)grid), dim3(ST), SLDS,
                           (hipStream_t)stream, y, row_off, idx, G, B, ypq, n0q, coef, iters, tau, score, (float*)ws,
                           slot_floats, qrow_off, qidx);
        return fpm::check_launch(what);
    }
};
}  // namespace

extern "C" int fpm_coarse_score_stream(const float* y, const long* row_off, const int* idx, int G, int B,
                                       const float* yp, int n0, const float* coef, int iters, float tau, float* score,
                                       void* ws, long ws_bytes, void* stream) {
    return fpm::coarse_score_entry<Stream, float>("fpm_coarse_score_stream", y, row_off, idx, G, B, yp, n0, coef, iters, tau,
                                           score, ws, ws_bytes, stream);
}

extern "C" int fpm_coarse_score_stream_rows16(const void* y16, const long* row_off, const int* idx, int G, int B,
                                              const float* yp, int n0, const float* coef, int iters, float tau,
                                              float* score, void* ws, long ws_bytes, void* stream) {
    return fpm::coarse_score_entry<Stream, bf16_t>("fpm_coarse_score_stream_rows16", (const bf16_t*)y16, row_off, idx, G, B, yp,
                                           n0, coef, iters, tau, score, ws, ws_bytes, stream);
}

extern "C" int fpm_coarse_pairs_stream(const float* y, const long* row_off, const int* idx, int G, int B,
                                       const float* yq, const long* qrow_off, const int* qidx, int Q, const float* coef,
                                       int iters, float tau, float* score, void* ws, long ws_bytes, void* stream) {
    return fpm::coarse_pairs_entry<Stream, float>("fpm_coarse_pairs_stream", y, row_off, idx, G, B, yq, qrow_off, qidx, Q, coef,
                                           iters, tau, score, ws, ws_bytes, stream);
}

extern "C" int fpm_coarse_pairs_stream_rows16(const void* y16, const long* row_off, const int* idx, int G, int B,
                                              const float* yq, const long* qrow_off, const int* qidx, int Q,
                                              const float* coef, int iters, float tau, float* score, void* ws,
                                              long ws_bytes, void* stream) {
    return fpm::coarse_pairs_entry<Stream, bf16_t>("fpm_coarse_pairs_stream_rows16", (const bf16_t*)y16, row_off, idx, G, B, yq,
                                           qrow_off, qidx, Q, coef, iters, tau, score, ws, ws_bytes, stream);
}

extern "C" int fpm_coarse_score_stream_rows8(const void* y8, const float* s8, const long* row_off, const int* idx, int G,
                                             int B, const float* yp, int n0, const float* coef, int iters, float tau,
                                             float* score, void* ws, long ws_bytes, void* stream) {
    return fpm::coarse_score_entry<Stream, fp8_t>("fpm_coarse_score_stream_rows8",
                                                  rows8_t{(const unsigned char*)y8, s8}, row_off, idx, G, B, yp, n0,
                                                  coef, iters, tau, score, ws, ws_bytes, stream);
}

extern "C" int fpm_coarse_pairs_stream_rows8(const void* y8, const float* s8, const long* row_off, const int* idx, int G,
                                             int B, const float* yq, const long* qrow_off, const int* qidx, int Q,
                                             const float* coef, int iters, float tau, float* score, void* ws,
                                             long ws_bytes, void* stream) {
    return fpm::coarse_pairs_entry<Stream, fp8_t>("fpm_coarse_pairs_stream_rows8",
                                                  rows8_t{(const unsigned char*)y8, s8}, row_off, idx, G, B, yq,
                                                  qrow_off, qidx, Q, coef, iters, tau, score, ws, ws_bytes, stream);
}

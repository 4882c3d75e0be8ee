// AFA-U k regressor (reference ngm.py:386-412 over src/model/afau.py:54-300).
//
// With the reference's inputs R0 = 0 and C0 = one-hot (ngm.py:392-399):
//   row block: q = Wq R0 = 0, so the mixed score depends on the cost only:
//     score_h[i,j] = mix2_h . relu(mix1_h[1] * cost[i,j] + mix1_bias_h) + mix2_bias_h
//     out[i, h*16+d] = sum_j softmax_j(score_h[i,:]) * Wv[h*16+d, j]   (v = Wv C0, zero for j >= n2b)
//   col block: v = Wv R0 = 0, so the attention output is exactly 0 and o1 = IN(C0 + combine.bias).
// Kernels: the row-block cross-set attention, instance norm (optionally + residual, optionally
// fused with the max-pool over positions), and the 600->8->1 heads + sigmoid.
// The projections/FFN are MFMA GEMMs through fpm_gemm.
#include "fpm_common.h"
#include <cstdlib>
#include <type_traits>

namespace {

// Row-block cross-set attention: one workgroup per (pair, 16-row tile), 4 waves; wave wv owns the
// column quarter j in [wv*4*TJ, (wv+1)*4*TJ) of all 16 rows, lane l row l&15 and the columns
// j = base + 4t + (l>>4), t < TJ -- exactly the operand layout of the fp32 MFMA 16x16x4, so the
// softmax numerators feed P . V straight from registers.  The tile's costs stay in registers
// across the 16 heads; V comes from global (L2-resident Wv), prefetched one head ahead.
//
// Scores: with q = 0 the mixed score is a scalar function of the cost,
//   f_h(c) = sum_m w2[m] relu(w1[m] c + b1[m]) + b2,
// piecewise linear with <= 16 breakpoints t_m = -b1[m] / w1[m].  At start the block builds in LDS,
// for all 16 heads, the sorted breakpoints, the 17 segments' (A, B) with f = A + B c, and a
// 64-bucket table over c in [0, 1] (the Sinkhorn output's range): the segment at the bucket's left
// edge and the <= 4 breakpoints inside it.  A score is one bucket lookup, four compares and one
// fma instead of 48 VALU operations; costs outside [0, 1] and buckets with 5+ breakpoints take the
// 16-term sum.  (Rounding differs from the 16-term sum by O(ulp) of the terms.)
// Softmax per wave quarter with its own running max (flash-style); the four quarters' (max, sum,
// partial P.V) are merged through LDS, one barrier per head (double-buffered partials).
constexpr int AF_NB = 64;      // score-LUT buckets over [0, 1]

struct AfSmem {
    int lseg[16][AF_NB];
    float4 lbp[16][AF_NB];
    float segA[16][17], segB[16][17];
    float part[2][4][256];     // [buffer][wave][row * 16 + d]
    float2 rowms[2][4][16];    // [buffer][wave][row] (running max, sum)
    float traw[256], tsort[256];
};

// SPLIT (T = bf16): each output row is [hi | lo | hi] (3 x 256 bf16, hi = bf16(o), lo = bf16(o - hi)),
// the split operand of the near-fp32 combine product (weights packed [W_hi | W_hi | W_lo]).
template <typename T, int TJ, bool SPLIT = false>
__global__ __launch_bounds__(256) void afau_row_attn_kernel(const float* __restrict__ cost, long c_sb, long c_ld,
                                                            int n1max, int n2max, const int* __restrict__ n2,
                                                            const float* __restrict__ Wv, int emb,
                                                            const float* __restrict__ mix1w,
                                                            const float* __restrict__ mix1b,
                                                            const float* __restrict__ mix2w,
                                                            const float* __restrict__ mix2b, T* __restrict__ out,
                                                            int use_lut, float2* __restrict__ stats) {
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    __shared__ AfSmem S;
    const int b = blockIdx.x, i0 = blockIdx.y * 16, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n2b = n2[b];

    // ---- score LUTs of the 16 heads (LUT mode only)
    if (use_lut) {
    {
        const int hh = tid >> 4, m = tid & 15;
        const float w = mix1w[(hh * 2 + 1) * 16 + m];
        S.traw[tid] = w != 0.f ? -mix1b[hh * 16 + m] / w : INFINITY;
    }
    __syncthreads();
    {
        const int hh = tid >> 4, m = tid & 15;
        const float t = S.traw[tid];
        int r = 0;
        for (int k = 0; k < 16; ++k) {
            const float u = S.traw[hh * 16 + k];
            r += (u < t) || (u == t && k < m);
        }
        S.tsort[hh * 16 + r] = t;
    }
    __syncthreads();
    for (int k = tid; k < 16 * 17; k += 256) {            // segment sg of head hh: (tsort[sg-1], tsort[sg])
        const int hh = k / 17, sg = k - 17 * hh;
        const float lo = sg == 0 ? -INFINITY : S.tsort[hh * 16 + sg - 1];
        const float hi = sg == 16 ? INFINITY : S.tsort[hh * 16 + sg];
        const bool flo = lo > -INFINITY && lo < INFINITY, fhi = hi > -INFINITY && hi < INFINITY;
        const float rep = (flo && fhi) ? 0.5f * (lo + hi) : flo ? lo + 1.f : fhi ? hi - 1.f : 0.f;
        float A = mix2b[hh], Bc = 0.f;
        for (int m = 0; m < 16; ++m) {
            const float w = mix1w[(hh * 2 + 1) * 16 + m], bb = mix1b[hh * 16 + m], w2 = mix2w[hh * 16 + m];
            const bool act = w != 0.f ? (w * rep + bb > 0.f) : (bb > 0.f);
            if (act) {
                A = fmaf(w2, bb, A);
                Bc = fmaf(w2, w, Bc);
            }
        }
        S.segA[hh][sg] = A;
        S.segB[hh][sg] = Bc;
    }
#pragma unroll
    for (int q = 0; q < 16 * AF_NB / 256; ++q) {          // bucket bk of head hh
        const int k = tid + 256 * q, hh = k / AF_NB, bk = k % AF_NB;
        const float lo = (float)bk / AF_NB, hi = (float)(bk + 1) / AF_NB;
        int s0 = 0, nin = 0;
        float bp[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
        for (int m = 0; m < 16; ++m) {
            const float t = S.tsort[hh * 16 + m];
            s0 += t < lo;
            if (t >= lo && t < hi) {
                if (nin < 4) bp[nin] = t;
                ++nin;
            }
        }
        S.lseg[hh][bk] = nin > 4 ? -1 : s0;
        S.lbp[hh][bk] = make_float4(bp[0], bp[1], bp[2], bp[3]);
    }
    __syncthreads();
    }

    // ---- costs and the first head's V (B operand: V[j][d], d = lane & 15)
    const int r = lane & 15, i = i0 + r, jbase = wv * 4 * TJ + (lane >> 4);
    const float* Cb = cost + (long)b * c_sb + (long)i * c_ld;
    float creg[TJ], vreg[TJ];
#pragma unroll
    for (int t = 0; t < TJ; ++t) {
        const int j = jbase + 4 * t;
        creg[t] = (i < n1max && j < n2max) ? Cb[j] : 0.f;
        vreg[t] = j < n2b ? Wv[(long)r * emb + j] : 0.f;
    }
    typedef float f2v __attribute__((ext_vector_type(2)));
    for (int h = 0; h < 16; ++h) {
        float p[TJ];
        float mloc = -INFINITY;
        if (!use_lut) {
            // the 16-term sum, m outer: the head's 48 weights are wave-uniform (scalar operands),
            // element pairs on v_pk_fma_f32; per element the same fma chain as the scalar form
            // sc = sum_m fma(relu(fma(c, w1, b1)), w2, sc) + b2 (no LDS lookups, no dependent loads)
            f2v acc2[TJ / 2];
#pragma unroll
            for (int t2 = 0; t2 < TJ / 2; ++t2) acc2[t2] = (f2v){0.f, 0.f};
            const float* w1p = mix1w + (h * 2 + 1) * 16;
            const float* b1p = mix1b + h * 16;
            const float* w2p = mix2w + h * 16;
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const float w1 = w1p[m], b1 = b1p[m], w2 = w2p[m];
#pragma unroll
                for (int t2 = 0; t2 < TJ / 2; ++t2) {
                    f2v u = (f2v){creg[2 * t2], creg[2 * t2 + 1]} * w1 + b1;
                    u.x = fmaxf(u.x, 0.f);
                    u.y = fmaxf(u.y, 0.f);
                    acc2[t2] = u * w2 + acc2[t2];
                }
            }
            const float b2 = mix2b[h];
#pragma unroll
            for (int t2 = 0; t2 < TJ / 2; ++t2) {
                p[2 * t2] = acc2[t2].x + b2;
                p[2 * t2 + 1] = acc2[t2].y + b2;
            }
#pragma unroll
            for (int t = 0; t < TJ; ++t)
                if (jbase + 4 * t < n2max) mloc = fmaxf(mloc, p[t]);
        } else
#pragma unroll
        for (int t = 0; t < TJ; ++t) {
            const float c = creg[t];
            float sc;
            int s0 = -1;
            float4 bp;
            if (use_lut && c >= 0.f && c <= 1.f) {
                const int bk = min((int)(c * AF_NB), AF_NB - 1);
                s0 = S.lseg[h][bk];
                bp = S.lbp[h][bk];
            }
            if (s0 >= 0) {
                const int sg = s0 + (bp.x < c) + (bp.y < c) + (bp.z < c) + (bp.w < c);
                sc = fmaf(S.segB[h][sg], c, S.segA[h][sg]);
            } else {
                sc = 0.f;
#pragma unroll 1
                for (int m = 0; m < 16; ++m)
                    sc += fmaxf(c * mix1w[(h * 2 + 1) * 16 + m] + mix1b[h * 16 + m], 0.f) * mix2w[h * 16 + m];
                sc += mix2b[h];
            }
            p[t] = sc;
            if (jbase + 4 * t < n2max) mloc = fmaxf(mloc, sc);
        }
        mloc = fpm::pair32_max(fpm::pair16_max(mloc));     // lane ^ 16, ^ 32 on the VALU
        float sloc = 0.f;
#pragma unroll
        for (int t = 0; t < TJ; ++t) {
            const float e = jbase + 4 * t < n2max ? fpm::fast_exp2((p[t] - mloc) * fpm::LOG2E_F) : 0.f;
            p[t] = e;
            sloc += e;
        }
        sloc = fpm::pair32_sum(fpm::pair16_sum(sloc));
        // unnormalised P . V over this wave's columns
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < TJ; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(p[t], vreg[t], acc, 0, 0, 0);
        if (h + 1 < 16) {                                 // next head's V
#pragma unroll
            for (int t = 0; t < TJ; ++t) {
                const int j = jbase + 4 * t;
                vreg[t] = j < n2b ? Wv[(long)((h + 1) * 16 + r) * emb + j] : 0.f;
            }
        }
        const int buf = h & 1;
#pragma unroll
        for (int k = 0; k < 4; ++k) S.part[buf][wv][(4 * (lane >> 4) + k) * 16 + r] = acc[k];
        if (lane < 16) S.rowms[buf][wv][lane] = make_float2(mloc, sloc);
        // LDS-only barrier: __syncthreads() would also wait for the next head's V loads just
        // issued and for this head's output stores (vmcnt(0)), exposing their latency every head
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        {
            const int rr = tid >> 4, d = tid & 15, ii = i0 + rr;
            float M = -INFINITY;
#pragma unroll
            for (int w = 0; w < 4; ++w) M = fmaxf(M, S.rowms[buf][w][rr].x);
            float o = 0.f, sum = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const float2 ms = S.rowms[buf][w][rr];
                const float sc = fpm::fast_exp2((ms.x - M) * fpm::LOG2E_F);
                sum = fmaf(ms.y, sc, sum);
                o = fmaf(S.part[buf][w][tid], sc, o);
            }
            if (stats && d == 0 && ii < n1max) stats[((long)b * n1max + ii) * 16 + h] = make_float2(M, sum);
            if (ii < n1max) {
                const float v = o / sum;
                if constexpr (SPLIT) {
                    T* orow = out + ((long)b * n1max + ii) * 768 + h * 16 + d;
                    const bf16_t hi = fpm::f2bf(v);
                    orow[0] = hi;
                    orow[256] = fpm::f2bf(v - fpm::bf2f(hi));
                    orow[512] = hi;
                } else {
                    out[((long)b * n1max + ii) * 256 + h * 16 + d] = fpm::from_f<T>(v);
                }
            }
        }
    }
}

// The same attention for n2max <= 256 with the 16-term scores (no LUT) and V staged in LDS.
// afau_row_attn_kernel reads its B operand V[j][d] = Wv[h*16 + d][j] straight from global memory,
// 16 B of each of 16 rows per load instruction (16 cache lines per wave instruction, every line
// touched 8 times per head): an L2-request-bound gather that held the kernel at ~10 % VALU issue.
// Here each head's 16 x 256 slice of Wv is copied once per workgroup with 16-B coalesced loads
// (issued one head ahead, written to the other LDS buffer after the head's MFMAs), and a lane's
// 16 B-operand values are 4 ds_read_b128 (rows padded to 260 floats: conflict-free).  Lane group
// q = lane >> 4 of wave wv owns the 16 CONTIGUOUS columns j = wv*64 + q*16 + t (the other kernel
// interleaves them with stride 4), so the costs are 16-B loads too; the P . V sum over j runs in
// a different order (fp32 rounding only).
// Heads: blockIdx.z of gridDim.z takes heads [16 z / Z, 16 (z + 1) / Z) -- small batches (a one-chunk
// forward's tail groups) split each 16-row block's head loop over Z workgroups so the launch fills
// the CUs; every (row, head) output is computed the same way whatever Z is (bit-identical).
template <typename T, bool SPLIT, bool FAST, int TJ = 16>
__global__ __launch_bounds__(256) void afau_row_attn_v_kernel(const float* __restrict__ cost, long c_sb, long c_ld,
                                                              int n1max, int n2max, const int* __restrict__ n2,
                                                              const float* __restrict__ Wv, int emb,
                                                              const float* __restrict__ mix1w,
                                                              const float* __restrict__ mix1b,
                                                              const float* __restrict__ mix2w,
                                                              const float* __restrict__ mix2b, T* __restrict__ out,
                                                              float2* __restrict__ stats) {
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    typedef float f2v __attribute__((ext_vector_type(2)));
    constexpr int VS = 16 * TJ + 4;                       // padded V row (floats)
    __shared__ __attribute__((aligned(16))) float vbuf[2][16 * VS];
    // per-wave partial outputs, element (row, d) at row * 16 + d + (row / 4) * 16: the four lane
    // groups of a wave write rows 4q + k (k fixed per instruction) into distinct banks
    __shared__ float part[2][4][320];
    __shared__ float2 rowms[2][4][16];
    const int b = blockIdx.x, i0 = blockIdx.y * 16, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n2b = n2[b];
    const int r = lane & 15, i = i0 + r, jl = wv * 4 * TJ + (lane >> 4) * TJ;

    // V staging: thread copies row vr, columns [vc, vc + TJ) of the head's slice (zero past n2b),
    // its TJ / 4 16-B chunks in an order rotated by (lane / 4) % 4: the 16 lanes of one row then
    // write 16 distinct 4-bank groups per ds_write_b128 (in order they hit 4 groups 4 times)
    const int vr = tid >> 4, vc = (tid & 15) * TJ, rot = (tid >> 2) & 3;
    float4 vnext[TJ / 4];
    auto vchunk = [&](int k) { return (k & ~3) | ((k + rot) & 3); };
    auto load_v = [&](int h) {
        const float* src = Wv + (long)(h * 16 + vr) * emb + vc;
#pragma unroll
        for (int k0 = 0; k0 < TJ / 4; ++k0) {
            const int k = vchunk(k0);
            const int j = vc + 4 * k;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j + 3 < n2b) {                            // n2b <= n2max <= emb: inside the row
                v = *(const float4*)(src + 4 * k);
            } else if (j < n2b) {
                v.x = src[4 * k];
                if (j + 1 < n2b) v.y = src[4 * k + 1];
                if (j + 2 < n2b) v.z = src[4 * k + 2];
            }
            vnext[k0] = v;
        }
    };
    auto store_v = [&](int buf) {
        float* dst = &vbuf[buf][vr * VS + vc];
#pragma unroll
        for (int k0 = 0; k0 < TJ / 4; ++k0) *(float4*)(dst + 4 * vchunk(k0)) = vnext[k0];
    };
    const int h0 = 16 * blockIdx.z / gridDim.z, h1 = 16 * (blockIdx.z + 1) / gridDim.z;
    load_v(h0);
    // costs: this lane's 16 contiguous columns of row i
    float creg[TJ];
    {
        const float* Cb = cost + (long)b * c_sb + (long)i * c_ld + jl;
        const bool vec = i < n1max && jl + TJ <= n2max && (((uintptr_t)Cb) & 15) == 0;
        if (vec) {
#pragma unroll
            for (int k = 0; k < TJ / 4; ++k) {
                const float4 c4 = *(const float4*)(Cb + 4 * k);
                creg[4 * k] = c4.x; creg[4 * k + 1] = c4.y; creg[4 * k + 2] = c4.z; creg[4 * k + 3] = c4.w;
            }
        } else {
#pragma unroll
            for (int t = 0; t < TJ; ++t) creg[t] = (i < n1max && jl + t < n2max) ? Cb[t] : 0.f;
        }
    }
    store_v(0);
    // FAST (bf16 modes): the wave's cost range [cmin, cmax]; a hidden unit m whose pre-activation
    // fma(c, w1, b1) has one sign at both ends (fma is monotone in c) is active or inactive for every
    // cost of the wave, so its relu term is linear (summed into A + B c once per head) or zero; only
    // units with a breakpoint inside the range are evaluated per element.  Exact up to fp32
    // reassociation (the fp32 parity mode keeps the per-element 16-term chain).
    float cmin = INFINITY, cmax = -INFINITY;
    if (FAST) {
#pragma unroll
        for (int t = 0; t < TJ; ++t) {
            cmin = fminf(cmin, creg[t]);
            cmax = fmaxf(cmax, creg[t]);
        }
        cmin = -fpm::warp_max(-cmin);                      // exact: min / max in any order
        cmax = fpm::warp_max(cmax);
    }
    __syncthreads();
    for (int h = h0; h < h1; ++h) {
        if (h + 1 < h1) load_v(h + 1);                    // lands during this head's scores
        float p[TJ];
        float mloc = -INFINITY;
        if (FAST) {
            const float* w1p = mix1w + (h * 2 + 1) * 16;
            const float* b1p = mix1b + h * 16;
            const float* w2p = mix2w + h * 16;
            float A = mix2b[h], Bl = 0.f;
            f2v acc2[TJ / 2];
#pragma unroll
            for (int t2 = 0; t2 < TJ / 2; ++t2) acc2[t2] = (f2v){0.f, 0.f};
            // the head's 48 weights in one batch of scalar loads (a rolled loop paid one scalar-load
            // latency per unit: ~800 dependent s_loads per wave)
            float w1a[16], b1a[16], w2a[16];
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                w1a[m] = w1p[m];
                b1a[m] = b1p[m];
                w2a[m] = w2p[m];
            }
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const float w1 = w1a[m], b1 = b1a[m], w2 = w2a[m];
                const float lo = fmaf(cmin, w1, b1), hi = fmaf(cmax, w1, b1);
                if (lo > 0.f && hi > 0.f) {               // active for the whole range
                    A = fmaf(w2, b1, A);
                    Bl = fmaf(w2, w1, Bl);
                } else if (lo > 0.f || hi > 0.f) {        // breakpoint inside: per element
#pragma unroll
                    for (int t2 = 0; t2 < TJ / 2; ++t2) {
                        f2v u = (f2v){creg[2 * t2], creg[2 * t2 + 1]} * w1 + b1;
                        u.x = fmaxf(u.x, 0.f);
                        u.y = fmaxf(u.y, 0.f);
                        acc2[t2] = u * w2 + acc2[t2];
                    }
                }
            }
#pragma unroll
            for (int t2 = 0; t2 < TJ / 2; ++t2) {
                p[2 * t2] = fmaf(Bl, creg[2 * t2], A) + acc2[t2].x;
                p[2 * t2 + 1] = fmaf(Bl, creg[2 * t2 + 1], A) + acc2[t2].y;
            }
#pragma unroll
            for (int t = 0; t < TJ; ++t)
                if (jl + t < n2max) mloc = fmaxf(mloc, p[t]);
        } else {
            f2v acc2[TJ / 2];
#pragma unroll
            for (int t2 = 0; t2 < TJ / 2; ++t2) acc2[t2] = (f2v){0.f, 0.f};
            const float* w1p = mix1w + (h * 2 + 1) * 16;
            const float* b1p = mix1b + h * 16;
            const float* w2p = mix2w + h * 16;
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const float w1 = w1p[m], b1 = b1p[m], w2 = w2p[m];
#pragma unroll
                for (int t2 = 0; t2 < TJ / 2; ++t2) {
                    f2v u = (f2v){creg[2 * t2], creg[2 * t2 + 1]} * w1 + b1;
                    u.x = fmaxf(u.x, 0.f);
                    u.y = fmaxf(u.y, 0.f);
                    acc2[t2] = u * w2 + acc2[t2];
                }
            }
            const float b2 = mix2b[h];
#pragma unroll
            for (int t2 = 0; t2 < TJ / 2; ++t2) {
                p[2 * t2] = acc2[t2].x + b2;
                p[2 * t2 + 1] = acc2[t2].y + b2;
            }
#pragma unroll
            for (int t = 0; t < TJ; ++t)
                if (jl + t < n2max) mloc = fmaxf(mloc, p[t]);
        }
        mloc = fpm::pair32_max(fpm::pair16_max(mloc));     // lane ^ 16, ^ 32 on the VALU
        float sloc = 0.f;
#pragma unroll
        for (int t = 0; t < TJ; ++t) {
            const float e = jl + t < n2max ? fpm::fast_exp2((p[t] - mloc) * fpm::LOG2E_F) : 0.f;
            p[t] = e;
            sloc += e;
        }
        sloc = fpm::pair32_sum(fpm::pair16_sum(sloc));
        const int buf = (h - h0) & 1;
        float vreg[TJ];
        {
            const float* vs = &vbuf[buf][r * VS + jl];
#pragma unroll
            for (int k = 0; k < TJ / 4; ++k) {
                const float4 v4 = *(const float4*)(vs + 4 * k);
                vreg[4 * k] = v4.x; vreg[4 * k + 1] = v4.y; vreg[4 * k + 2] = v4.z; vreg[4 * k + 3] = v4.w;
            }
        }
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < TJ; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(p[t], vreg[t], acc, 0, 0, 0);
        if (h + 1 < h1) store_v(buf ^ 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) part[buf][wv][(4 * (lane >> 4) + k) * 16 + r + (lane >> 4) * 16] = acc[k];
        if (lane < 16) rowms[buf][wv][lane] = make_float2(mloc, sloc);
        // LDS-only barrier (no vmcnt(0): this head's output stores stay in flight)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        {
            const int rr = tid >> 4, d = tid & 15, ii = i0 + rr;
            float M = -INFINITY;
#pragma unroll
            for (int w = 0; w < 4; ++w) M = fmaxf(M, rowms[buf][w][rr].x);
            float o = 0.f, sum = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const float2 ms = rowms[buf][w][rr];
                const float sc = fpm::fast_exp2((ms.x - M) * fpm::LOG2E_F);
                sum = fmaf(ms.y, sc, sum);
                o = fmaf(part[buf][w][tid + (rr >> 2) * 16], sc, o);
            }
            if (stats && d == 0 && ii < n1max) stats[((long)b * n1max + ii) * 16 + h] = make_float2(M, sum);
            if (ii < n1max) {
                const float v = o / sum;
                if constexpr (SPLIT) {
                    T* orow = out + ((long)b * n1max + ii) * 768 + h * 16 + d;
                    const bf16_t hi = fpm::f2bf(v);
                    orow[0] = hi;
                    orow[256] = fpm::f2bf(v - fpm::bf2f(hi));
                    orow[512] = hi;
                } else {
                    out[((long)b * n1max + ii) * 256 + h * 16 + d] = fpm::from_f<T>(v);
                }
            }
        }
    }
}

// InstanceNorm1d over positions (afau.py:145-176) of x = in1 (+ in2), or of the synthesised col
// input C0 + bias (onehot mode).  Writes out_f / out_t, or (gmax != null) only the max over
// positions of the normalised values (MaxPool1d over the -inf padded 600 positions, ngm.py:402-405).
// 1024 threads = 16 position groups x 64 channels; each thread keeps its <= NV values in registers,
// so x is read once (mean, variance and output from registers; position 0 once more, as the shift).
template <typename T, int NV>
__global__ __launch_bounds__(1024) void instnorm_kernel(const float* __restrict__ in1, const float* __restrict__ in2,
                                                        int P, int Cn, const int* __restrict__ nvalid,
                                                        const float* __restrict__ onehot_bias, const float* __restrict__ w,
                                                        const float* __restrict__ bb, float eps, float* __restrict__ out_f,
                                                        T* __restrict__ out_t, int ldt, float* __restrict__ gmax) {
    __shared__ float red[16][64];
    const int b = blockIdx.x, cl = threadIdx.x & 63, c = blockIdx.y * 64 + cl, g = threadIdx.x >> 6;
    const bool cv = c < Cn;
    const int nb = onehot_bias ? nvalid[b] : 0;
    // The values are kept relative to the channel's first position x0 (the norm is shift-invariant):
    // the mean of x - x0 rounds at the scale of the channel's spread, not of its offset.  A channel
    // without spread -- every column-block channel c >= n2 is the constant combine bias -- would
    // otherwise come out as rstd = 1 / sqrt(eps) = 316 times the rounding error of its fp32 mean.
    float x0 = 0.f;
    if (cv && P > 0) {
        if (onehot_bias) {
            x0 = ((c == 0 && nb > 0) ? 1.f : 0.f) + onehot_bias[c];
        } else {
            const long o = (long)b * P * Cn + c;
            x0 = in2 ? in1[o] + in2[o] : in1[o];
        }
    }
    float v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int p = g + 16 * k;
        float x = 0.f;
        if (cv && p < P) {
            if (onehot_bias) {
                x = ((p == c && p < nb) ? 1.f : 0.f) + onehot_bias[c];
            } else {
                const long o = ((long)b * P + p) * Cn + c;
                x = in2 ? in1[o] + in2[o] : in1[o];
            }
            x -= x0;
        }
        v[k] = x;
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) s += v[k];
    red[g][cl] = s;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) tot += red[q][cl];
    const float mean = tot / (float)P;
    __syncthreads();
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int p = g + 16 * k;
        const float d = v[k] - mean;
        if (p < P) sq += d * d;
    }
    red[g][cl] = sq;
    __syncthreads();
    float var = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) var += red[q][cl];
    var /= (float)P;
    const float rstd = 1.f / sqrtf(var + eps);
    const float ww = cv ? w[c] : 0.f, bv = cv ? bb[c] : 0.f;
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int p = g + 16 * k;
        if (!cv || p >= P) continue;
        const float y = (v[k] - mean) * rstd * ww + bv;
        if (gmax) mx = fmaxf(mx, y);
        else {
            const long o = ((long)b * P + p) * Cn + c;
            if (out_f) out_f[o] = y;
            if (out_t) out_t[((long)b * P + p) * ldt + c] = fpm::from_f<T>(y);
        }
    }
    // zero K-padding columns [Cn, ldt) of the operand copy (the next GEMM runs K = ldt)
    if (!cv && out_t && !gmax && c < ldt)
        for (int p = g; p < P; p += 16) out_t[((long)b * P + p) * ldt + c] = fpm::from_f<T>(0.f);
    if (gmax) {
        __syncthreads();
        red[g][cl] = mx;
        __syncthreads();
        if (g == 0 && cv) {
            float m = red[0][cl];
#pragma unroll
            for (int q = 1; q < 16; ++q) m = fmaxf(m, red[q][cl]);
            gmax[(long)b * Cn + c] = m;
        }
    }
}

// ks = sigmoid((final_row(gr) + final_col(gc)) / 2)   (ngm.py:406-412, mean_k = True): the 8
// hidden units on 8 waves (a one-wave form ran the 16 dot products of length E back to back:
// ~60 us per launch, latency-bound on 1 wave per pair); the units combined in order by thread 0.
__global__ __launch_bounds__(512) void afau_head8_kernel(const float* __restrict__ gr, const float* __restrict__ gc,
                                                         int E, const float* __restrict__ r0w, const float* __restrict__ r0b,
                                                         const float* __restrict__ r2w, const float* __restrict__ r2b,
                                                         const float* __restrict__ c0w, const float* __restrict__ c0b,
                                                         const float* __restrict__ c2w, const float* __restrict__ c2b,
                                                         float* __restrict__ ks) {
    __shared__ float hid[2][8];
    const int b = blockIdx.x, lane = threadIdx.x & 63, m = threadIdx.x >> 6;
    float sr = 0.f, sc = 0.f;
    for (int k = lane; k < E; k += 64) {
        sr += r0w[m * E + k] * gr[(long)b * E + k];
        sc += c0w[m * E + k] * gc[(long)b * E + k];
    }
    sr = fpm::warp_sum(sr) + r0b[m];
    sc = fpm::warp_sum(sc) + c0b[m];
    if (lane == 0) {
        hid[0][m] = sr;
        hid[1][m] = sc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float kr = 0.f, kc = 0.f;
        for (int u = 0; u < 8; ++u) {
            kr += r2w[u] * fmaxf(hid[0][u], 0.f);
            kc += c2w[u] * fmaxf(hid[1][u], 0.f);
        }
        kr += r2b[0];
        kc += c2b[0];
        ks[b] = 1.f / (1.f + expf(-((kr + kc) / 2.f)));
    }
}

}  // namespace

// the LDS-staged-V kernel where it applies (1) or always the gather kernel (0): kernel-vs-kernel
// tests only, fpm_set_tuning("afau_attn_v", v)
int& afau_attn_v_flag() {
    static int v = 1;
    return v;
}

// heads per row block split over gridDim.z workgroups: 0 = by launch size (above), 1/2/4/8/16 forced
// (fpm_set_tuning("afau_head_split", z); same results)
int& afau_head_split_flag() {
    static int v = 0;
    return v;
}

extern "C" int fpm_crossset_attn_fwd(int dtype, const float* cost, long c_sb, long c_ld, int B, int n1max, int n2max,
                                     const int* n2, const float* Wv, int emb, const float* mix1w, const float* mix1b,
                                     const float* mix2w, const float* mix2b, void* out, float* stats, void* stream) {
    FPM_CHECK_ARG(n2max <= emb, "crossset_attn: n2max > embedding dim");
    if (B == 0) return 0;
    dim3 grid(B, (n1max + 15) / 16);
    hipStream_t st = (hipStream_t)stream;
    FPM_CHECK_ARG(n2max <= 640, "crossset_attn: n2max %d > 640", n2max);
    // the LDS-staged-V kernel where it applies (n2max <= 512); beyond, the gather kernel, whose
    // bf16 throughput modes score through a lookup table (fp32 parity mode: the 16-term sum, the
    // reference's operation order)
    const bool v_ok = n2max <= 512 && emb >= n2max && emb % 4 == 0 && ((uintptr_t)Wv & 15) == 0 && afau_attn_v_flag();
    const int lut = dtype != 0 && !v_ok;
#define FPM_ATT(TT, TJ_, SP_)                                                                                    \
    hipLaunchKernelGGL((afau_row_attn_kernel<TT, TJ_, SP_>), grid, dim3(256), 0, st, cost, c_sb, c_ld, n1max, n2max, \
                       n2, Wv, emb, mix1w, mix1b, mix2w, mix2b, (TT*)out, lut, (float2*)stats)
    const bool vpath = v_ok;
    // head split for small launches: fewer than ~8 workgroups per CU (256 CUs) leave each CU's one or
    // two workgroups latency-bound through their 16 sequential heads
    dim3 gridv = grid;
    {
        const long wgs = (long)grid.x * grid.y;
        gridv.z = wgs >= 2048 ? 1 : wgs >= 1024 ? 2 : wgs >= 512 ? 4 : 8;
        if (afau_head_split_flag() > 0) gridv.z = afau_head_split_flag();
    }
#define FPM_ATTV(TT, SP_)                                                                                        \
    do {                                                                                                         \
        if (n2max <= 256)                                                                                        \
            hipLaunchKernelGGL((afau_row_attn_v_kernel<TT, SP_, !std::is_same<TT, float>::value, 16>), gridv,    \
                               dim3(256), 0, st, cost, c_sb, c_ld, n1max, n2max, n2, Wv, emb, mix1w, mix1b,      \
                               mix2w, mix2b, (TT*)out, (float2*)stats);                                          \
        else                                                                                                     \
            hipLaunchKernelGGL((afau_row_attn_v_kernel<TT, SP_, !std::is_same<TT, float>::value, 32>), gridv,    \
                               dim3(256), 0, st, cost, c_sb, c_ld, n1max, n2max, n2, Wv, emb, mix1w, mix1b,      \
                               mix2w, mix2b, (TT*)out, (float2*)stats);                                          \
    } while (0)
    if (vpath) {
        if (dtype == 0) FPM_ATTV(float, false);
        else if (dtype == 1) FPM_ATTV(bf16_t, false);
        else FPM_ATTV(bf16_t, true);
        return fpm::check_launch("fpm_crossset_attn_fwd");
    }
#undef FPM_ATTV
    if (dtype == 0) { if (n2max <= 256) FPM_ATT(float, 16, false); else FPM_ATT(float, 40, false); }
    else if (dtype == 1) { if (n2max <= 256) FPM_ATT(bf16_t, 16, false); else FPM_ATT(bf16_t, 40, false); }
    else { if (n2max <= 256) FPM_ATT(bf16_t, 16, true); else FPM_ATT(bf16_t, 40, true); }
#undef FPM_ATT
    return fpm::check_launch("fpm_crossset_attn_fwd");
}

extern "C" int fpm_instnorm(int dtype, const float* in1, const float* in2, int B, int P, int Cn, const int* nvalid,
                            const float* onehot_bias, const float* w, const float* bias, float eps, float* out_f,
                            void* out_t, int ldt, float* gmax, void* stream) {
    if (B == 0) return 0;
    if (ldt <= 0) ldt = Cn;
    FPM_CHECK_ARG(ldt >= Cn, "instnorm: ldt %d < Cn %d", ldt, Cn);
    const int cols = ldt > Cn ? ldt : Cn;
    dim3 grid(B, (cols + 63) / 64);
    FPM_CHECK_ARG(P <= 640, "instnorm: P=%d > 640 positions", P);
    hipStream_t st = (hipStream_t)stream;
#define FPM_IN(TT, NV)                                                                                     \
    hipLaunchKernelGGL((instnorm_kernel<TT, NV>), grid, dim3(1024), 0, st, in1, in2, P, Cn, nvalid, onehot_bias, w, \
                       bias, eps, out_f, (TT*)out_t, ldt, gmax)
    if (dtype == 0) { if (P <= 256) FPM_IN(float, 16); else FPM_IN(float, 40); }
    else { if (P <= 256) FPM_IN(bf16_t, 16); else FPM_IN(bf16_t, 40); }
#undef FPM_IN
    return fpm::check_launch("fpm_instnorm");
}

extern "C" int fpm_afau_head(const float* gr, const float* gc, int B, int E, const float* r0w, const float* r0b,
                             const float* r2w, const float* r2b, const float* c0w, const float* c0b, const float* c2w,
                             const float* c2b, float* ks, void* stream) {
    if (B == 0) return 0;
    hipLaunchKernelGGL(afau_head8_kernel, dim3(B), dim3(512), 0, (hipStream_t)stream, gr, gc, E, r0w, r0b, r2w, r2b,
                       c0w, c0b, c2w, c2b, ks);
    return fpm::check_launch("fpm_afau_head");
}

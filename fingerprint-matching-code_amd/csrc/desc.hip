// Prescreen descriptors of a 1:N identification: one fixed-length vector per template, scored against every
// entry of the index at memory bandwidth before the coarse pass sees any of them.
//
//   fpm_rows_pool    the descriptor of an entry: its 768-channel index rows summed (fp32, rows ascending),
//                    L2-normalised in fp64, rounded to bf16.  Every step is one correctly rounded IEEE operation
//                    in a fixed order (include/fpm.h states it), so ops.rows_pool's host statement gives the
//                    same bits.
//   fpm_desc_score   probes x entries dot products of such descriptors on v_mfma_f32_16x16x32_bf16.
#include "fpm_common.h"
#include "fpm.h"

namespace {
constexpr int DK = 768;
constexpr int PT = DK / 4;          // rows_pool: threads per entry, a float4 of channels each
constexpr int PRED = 256;           // rows_pool: the norm's tree runs over this many partial sums

__device__ __forceinline__ void add4(float4& m, const float4 v) {
    m.x = __fadd_rn(m.x, v.x);
    m.y = __fadd_rn(m.y, v.y);
    m.z = __fadd_rn(m.z, v.z);
    m.w = __fadd_rn(m.w, v.w);
}

__global__ __launch_bounds__(PT) void rows_pool_kernel(const float* __restrict__ y, long rows,
                                                       const long* __restrict__ row_off, int lo,
                                                       bf16_t* __restrict__ desc) {
    __shared__ double p[PRED];
    const int tid = threadIdx.x;
    const long g = (long)lo + blockIdx.x;
    const long o0 = row_off[g], o1 = row_off[g + 1];
    const bool ok = o0 >= 0 && o1 >= o0 && o1 <= rows;         // otherwise nothing is read
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) {
        const float4* src = (const float4*)(y + o0 * DK) + tid;
        const long n = o1 - o0;
        long i = 0;
        for (; i + 4 <= n; i += 4) {                           // four rows in flight, added in row order
            const float4 v0 = src[(i + 0) * PT], v1 = src[(i + 1) * PT], v2 = src[(i + 2) * PT],
                         v3 = src[(i + 3) * PT];
            add4(m, v0);
            add4(m, v1);
            add4(m, v2);
            add4(m, v3);
        }
        for (; i < n; ++i) add4(m, src[i * PT]);
    }
    const double dx = (double)m.x, dy = (double)m.y, dz = (double)m.z, dw = (double)m.w;
    p[tid] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)),
                       __dmul_rn(dw, dw));
    if (tid < PRED - PT) p[PT + tid] = 0.0;
    __syncthreads();
    for (int o = PRED / 2; o > 0; o >>= 1) {
        if (tid < o) p[tid] = __dadd_rn(p[tid], p[tid + o]);
        __syncthreads();
    }
    const double ss = p[0];
    uint2 out = make_uint2(0u, 0u);
    if (ok && ss > 0.0 && ss <= 1.7976931348623157e308) {      // not 0, not inf, not NaN
        const double r = __dsqrt_rn(ss);
        out.x = fpm::f2bf2((float)__ddiv_rn(dx, r), (float)__ddiv_rn(dy, r));
        out.y = fpm::f2bf2((float)__ddiv_rn(dz, r), (float)__ddiv_rn(dw, r));
    }
    *(uint2*)(desc + (long)blockIdx.x * DK + 4 * tid) = out;
}

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
constexpr int DSTEPS = DK / 32;     // K steps of the 16 x 16 x 32 MFMA
constexpr int DWAVES = 4;

// Lane l of a wave holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15], j < 8: for both
// operands that is 16 contiguous bytes of a descriptor, read straight from global memory.  A = the probe tile
// (kept in 96 registers for the whole launch), B = 16 entries; the four lanes of a row cover 64 contiguous bytes
// per step and every byte of the entry over the 24 steps.  D: col = l & 15 (entry), row = 4 (l >> 4) + reg (probe).
__global__ __launch_bounds__(64 * DWAVES) void desc_score_kernel(const bf16_t* __restrict__ dq, int Q,
                                                                 const bf16_t* __restrict__ dg, int G,
                                                                 const int* __restrict__ idx, int B,
                                                                 float* __restrict__ score) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = lane & 15, q4 = lane >> 4;
    const long probe = (long)blockIdx.y * 16 + r;
    bf16x8_t a[DSTEPS];
#pragma unroll
    for (int s = 0; s < DSTEPS; ++s) a[s] = (bf16x8_t)(0);
    if (probe < Q) {
        const bf16_t* src = dq + probe * DK + 8 * q4;
#pragma unroll
        for (int s = 0; s < DSTEPS; ++s) a[s] = *(const bf16x8_t*)(src + 32 * s);
    }
    const long tiles = ((long)B + 15) / 16;
    for (long t = (long)blockIdx.x * DWAVES + wv; t < tiles; t += (long)gridDim.x * DWAVES) {   // wave-uniform
        const long b = t * 16 + r;
        long e = -1;
        if (b < B) e = idx ? (long)idx[b] : b;
        const bool ok = e >= 0 && e < G;
        bf16x8_t bb[DSTEPS];
#pragma unroll
        for (int s = 0; s < DSTEPS; ++s) bb[s] = (bf16x8_t)(0);
        if (ok) {
            const bf16_t* src = dg + e * DK + 8 * q4;
#pragma unroll
            for (int s = 0; s < DSTEPS; ++s) bb[s] = *(const bf16x8_t*)(src + 32 * s);
        }
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < DSTEPS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[s], bb[s], acc, 0, 0, 0);
        if (b < B) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long p = (long)blockIdx.y * 16 + 4 * q4 + j;
                if (p < Q) score[p * B + b] = ok ? acc[j] : __uint_as_float(0x7FC00000u);
            }
        }
    }
}
}  // namespace

extern "C" int fpm_rows_pool(const float* y, long rows, const long* row_off, int lo, int hi, void* desc,
                             void* stream) {
    FPM_CHECK_ARG(rows >= 0 && lo >= 0 && hi >= lo, "rows_pool: bad sizes (rows %ld, entries [%d, %d))", rows, lo, hi);
    if (hi == lo) return 0;
    FPM_CHECK_ARG(row_off && desc && (y || rows == 0), "rows_pool: y, row_off and desc are required");
    FPM_CHECK_ARG(((uintptr_t)y & 15) == 0 && ((uintptr_t)desc & 7) == 0 && ((uintptr_t)row_off & 7) == 0,
                  "rows_pool: y must be 16-byte aligned, desc and row_off 8-byte aligned");
    hipLaunchKernelGGL(rows_pool_kernel, dim3((unsigned)(hi - lo)), dim3(PT), 0, (hipStream_t)stream, y, rows, row_off,
                       lo, (bf16_t*)desc);
    return fpm::check_launch("fpm_rows_pool");
}

extern "C" int fpm_desc_score(const void* dq, int Q, const void* dg, int G, const int* idx, int B, float* score,
                              void* stream) {
    FPM_CHECK_ARG(Q >= 0 && G >= 0 && B >= 0, "desc_score: bad sizes (Q %d, G %d, B %d)", Q, G, B);
    FPM_CHECK_ARG(idx || B == G, "desc_score: without idx every entry is scored in order (B %d, G %d)", B, G);
    FPM_CHECK_ARG(Q <= 16 * 65535, "desc_score: at most %d probes per call (Q %d)", 16 * 65535, Q);
    if (Q == 0 || B == 0) return 0;
    FPM_CHECK_ARG(dq && score && (dg || G == 0), "desc_score: dq, dg and score are required");
    FPM_CHECK_ARG((((uintptr_t)dq | (uintptr_t)dg) & 15) == 0 && ((uintptr_t)score & 3) == 0 && ((uintptr_t)idx & 3) == 0,
                  "desc_score: dq and dg must be 16-byte aligned, score and idx 4-byte aligned");
    const long tiles = ((long)B + 15) / 16;
    long nb = (tiles + DWAVES - 1) / DWAVES;
    nb = nb > 4096 ? 4096 : nb;
    hipLaunchKernelGGL(desc_score_kernel, dim3((unsigned)nb, (unsigned)((Q + 15) / 16)), dim3(64 * DWAVES), 0,
                       (hipStream_t)stream, (const bf16_t*)dq, Q, (const bf16_t*)dg, G, idx, B, score);
    return fpm::check_launch("fpm_desc_score");
}

// Quantisation of index rows to fp8 (the "fp8+host" layout of a gallery index: what the coarse kernels'
// _rows8 entry points read).  A row y[r] of 768 fp32 values becomes 768 e4m3 bytes (OCP e4m3fn, gfx950's own
// encoding) and one fp32 scale, a power of two:
//
//     amax = max_k |y[r, k]|;  e = 0 if amax == 0, else the smallest e with amax <= 448 * 2^e, held to
//     [-110, 110];  s8[r] = 2^e;  y8[r, k] = e4m3(clamp(y[r, k] * 2^-e, -448, 448)), to nearest even.
//
// (ops.rows_quant8 states the same in torch.)  The scale being a power of two, float(y8) * s8 has four
// significant bits and, with e in [-110, 110], lies in bf16's normal range: the coarse operand
// bf16(float(y8) * s8) is exact.
//
// One wave per row, four rows per workgroup, one pass: a lane holds 12 values (three 16-B loads, lanes
// adjacent), the absolute maximum is taken on the values' bits as integers (the order of non-negative
// floats; no flush of a subnormal can change it) and over the wave by DPP, the exponent comes from the
// maximum's exponent and mantissa bits (amax = 1.m x 2^(E - 127) <= 448 x 2^e = 1.75 x 2^(e + 8): e = E - 135,
// one more when the mantissa is over .75; E = 0, a subnormal, lands below the lower bound as its true
// exponent does), y * 2^-e is one exact multiply, and the conversion is v_cvt_pk_fp8_f32.  Three 4-B stores
// per lane, lanes adjacent; lane 0 writes the scale.
#include "fpm_common.h"
#include "fpm.h"

namespace {
constexpr int QK = 768;
constexpr int QROWS = 4;      // rows (waves) per workgroup
constexpr int QEMAX = 110;    // |e| at most: float(y8) * 2^e stays a normal bf16 (2^-9 * 2^-110, 448 * 2^110)

__device__ __forceinline__ unsigned umax_dpp(unsigned v, unsigned o) { return v > o ? v : o; }
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
// the maximum over the wave, in every lane (the tree of fpm::warp_max, on unsigned integers)
__device__ __forceinline__ unsigned wave_umax(unsigned v) {
    v = umax_dpp(v, dpp_u<0xB1>(v));
    v = umax_dpp(v, dpp_u<0x4E>(v));
    v = umax_dpp(v, dpp_u<0x141>(v));
    v = umax_dpp(v, dpp_u<0x140>(v));
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    v = umax_dpp(r[0], r[1]);
    const auto q = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return umax_dpp(q[0], q[1]);
}

__device__ __forceinline__ float clamp448(float x) { return fminf(fmaxf(x, -448.f), 448.f); }

__global__ __launch_bounds__(64 * QROWS) void rows_quant8_kernel(const float* __restrict__ y, long rows,
                                                                 unsigned char* __restrict__ y8,
                                                                 float* __restrict__ s8) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * QROWS + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // wave-uniform
    const float4* src = (const float4*)(y + row * QK);
    float4 v[3];
    unsigned am = 0u;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        v[j] = src[lane + 64 * j];
        const unsigned a = __float_as_uint(v[j].x) & 0x7fffffffu, b = __float_as_uint(v[j].y) & 0x7fffffffu;
        const unsigned c = __float_as_uint(v[j].z) & 0x7fffffffu, d = __float_as_uint(v[j].w) & 0x7fffffffu;
        am = umax_dpp(am, umax_dpp(umax_dpp(a, b), umax_dpp(c, d)));
    }
    am = wave_umax(am);
    int e = 0;
    if (am != 0u) {
        e = (int)(am >> 23) - 135 + ((am & 0x7fffffu) > 0x600000u ? 1 : 0);
        e = e < -QEMAX ? -QEMAX : (e > QEMAX ? QEMAX : e);
    }
    const float inv = __uint_as_float((unsigned)(127 - e) << 23);   // 2^-e
    unsigned* dst = (unsigned*)(y8 + row * QK);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        int p = 0;
        p = __builtin_amdgcn_cvt_pk_fp8_f32(clamp448(__fmul_rn(v[j].x, inv)), clamp448(__fmul_rn(v[j].y, inv)), p,
                                            false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(clamp448(__fmul_rn(v[j].z, inv)), clamp448(__fmul_rn(v[j].w, inv)), p,
                                            true);
        dst[lane + 64 * j] = (unsigned)p;
    }
    if (lane == 0) s8[row] = __uint_as_float((unsigned)(127 + e) << 23);
}
}  // namespace

extern "C" int fpm_rows_quant8(const float* y, long rows, void* y8, float* s8, void* stream) {
    FPM_CHECK_ARG(rows >= 0 && rows <= 0x7fffffffL * QROWS, "rows_quant8: bad row count %ld", rows);
    if (rows == 0) return 0;
    FPM_CHECK_ARG(y && y8 && s8, "rows_quant8: y, y8 and s8 are required");
    FPM_CHECK_ARG((((uintptr_t)y | (uintptr_t)y8) & 15) == 0 && ((uintptr_t)s8 & 3) == 0,
                  "rows_quant8: y and y8 must be 16-byte aligned, s8 4-byte aligned");
    hipLaunchKernelGGL(rows_quant8_kernel, dim3((unsigned)((rows + QROWS - 1) / QROWS)), dim3(64 * QROWS), 0,
                       (hipStream_t)stream, y, rows, (unsigned char*)y8, s8);
    return fpm::check_launch("fpm_rows_quant8");
}

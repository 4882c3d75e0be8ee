// Device helpers shared by the three coarse-score kernels (coarse.hip, coarse_wide.hip,
// coarse_stream.hip): the vector types, the 16-lane maximum, the native softplus, the three forms of the
// entry rows (fp32, bf16, fp8 with a row scale), and the copy of one side's K tile from global memory into
// LDS, written once over the kernel's geometry.
#pragma once
#include "fpm_common.h"

namespace fpm {
namespace coarse {
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, fpm::dpp_f<0xB1>(v));
    v = fmaxf(v, fpm::dpp_f<0x4E>(v));
    v = fmaxf(v, fpm::dpp_f<0x141>(v));
    return fmaxf(v, fpm::dpp_f<0x140>(v));
}
// softplus = max(x, 0) + log1p(exp(-|x|)) on the native base-2 transcendentals, with log1p's classic
// correction for the rounding of 1 + t.  The libm pair (fpm::softplus_f) is ~150 instructions per
// element, 128 elements per thread in the wide kernel: it was a third of that kernel's time.  Measured
// against float64 over N(0, 0.05 .. 4) arguments: mean error 2.7e-8 .. 4.2e-8, the libm pair's
// 2.4e-8 .. 4.4e-8 (the result's own rounding dominates both).  x > 20: t < 2^-28, the sum rounds to x,
// torch's threshold.
__device__ __forceinline__ float softplus_native(float x) {
    const float t = fpm::fast_exp2(-fabsf(x) * fpm::LOG2E_F);
    const float u = 1.f + t;
    const float c = (t - (u - 1.f)) * __builtin_amdgcn_rcpf(u);
    return fmaxf(x, 0.f) + (fpm::fast_log2(u) * fpm::LN2_F + c);
}
// a finite stand-in for the maximum of an all -inf set (exp2(-inf - 0) = 0: an empty sum)
__device__ __forceinline__ float finite_max(float m) { return m == -INFINITY ? 0.f : m; }

constexpr int log2_of(int v) { return v <= 1 ? 0 : 1 + log2_of(v >> 1); }

// The entry rows as a kernel takes them.  fp32 and bf16 rows: a pointer to YT.  fp8 rows (the _rows8 entry
// points: an index that keeps e4m3 bytes and one power-of-two fp32 scale per row, ops.rows_quant8): the tag
// type fp8_t stands for them and the kernel's argument is the pair of pointers, so that the fp32 and bf16
// instantiations keep the argument list, and with it the registers, that they had.
struct fp8_t {
    unsigned char v;
};
struct rows8_t {
    const unsigned char* y;   // (rows, 768) e4m3 (OCP: gfx950's own encoding)
    const float* s;           // (rows,) 2^e
};
template <typename YT>
struct EntryRows {
    typedef const YT* __restrict__ arg;
    typedef const YT* host;
};
template <>
struct EntryRows<fp8_t> {
    typedef rows8_t arg;
    typedef rows8_t host;
};
// y + o: the rows from channel offset o (a multiple of 768) on, as for a pointer to fp32 or bf16 rows
__device__ __forceinline__ rows8_t operator+(rows8_t y, long o) { return rows8_t{y.y + o, y.s + o / 768}; }
inline bool rows_given(const void* y) { return y != nullptr; }
inline bool rows_given(rows8_t y) { return y.y != nullptr && y.s != nullptr; }

// One side's K tile of a workgroup of T threads: BK channels of up to NM passes of rows, each operand
// row ROW bytes apart in LDS (BK bf16 + padding).  A thread's place is written as a shift and a mask of
// tid, never a division: tid may be a value the compiler cannot prove non-negative (coarse_wide.hip's
// fresh_pos), and a signed division there costs the kernel thousands of instructions.
template <int T, int BK, int ROW>
struct Tile {
    static constexpr int CK = 768;                           // channels
    // fp32 rows: a float4 per thread and pass, BK / 4 threads along a row, T / (BK / 4) rows per pass
    static constexpr int SH = log2_of(BK / 4), RP = T >> SH;
    // bf16 rows: 8 bf16 per thread and pass, BK / 8 threads along a row
    static constexpr int SH16 = log2_of(BK / 8), RP16 = T >> SH16;
    static_assert((4 << SH) == BK && (8 << SH16) == BK && (RP << SH) == T, "powers of two: shift and mask");

    // this thread's NM float4 (rows row_base + (tid >> SH) + RP m, columns 4 (tid & (BK / 4 - 1)) ..), zeros
    // past n without a read
    template <int NM>
    static __device__ __forceinline__ void load(const float* __restrict__ base, int n, int row_base, int k0, int tid,
                                                float4 (&r)[NM]) {
        const int row0 = row_base + (tid >> SH), c = 4 * (tid & (BK / 4 - 1));
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const int row = row0 + RP * m;
            r[m] = row < n ? *(const float4*)(base + (long)row * CK + k0 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    // scale (one fp32 multiply; the unscaled side multiplies by 1, exactly), round to bf16, into LDS
    template <int NM>
    static __device__ __forceinline__ void store(unsigned char* tile, int tid, const float4 (&r)[NM], float4 s) {
        const int row0 = tid >> SH, c = 4 * (tid & (BK / 4 - 1));
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            uint2 o;
            o.x = fpm::f2bf2(__fmul_rn(r[m].x, s.x), __fmul_rn(r[m].y, s.y));
            o.y = fpm::f2bf2(__fmul_rn(r[m].z, s.z), __fmul_rn(r[m].w, s.w));
            *(uint2*)(tile + (row0 + RP * m) * ROW + c * 2) = o;
        }
    }
    // the entry's K tile from bf16 rows (the _rows16 entry points: an index that keeps a bf16 copy of its
    // rows, the same RNE rounding done once at enrolment): this thread's NM vectors of 8 bf16 (rows
    // row_base + (tid >> SH16) + RP16 m, columns 8 (tid & (BK / 8 - 1)) ..; a row is 1536 B, so every
    // vector is 16-B aligned), zeros past n
    template <int NM>
    static __device__ __forceinline__ void load16(const bf16_t* __restrict__ base, int n, int row_base, int k0, int tid,
                                                  uint4 (&r)[NM]) {
        const int row0 = row_base + (tid >> SH16), c = 8 * (tid & (BK / 8 - 1));
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const int row = row0 + RP16 * m;
            r[m] = row < n ? *(const uint4*)(base + (long)row * CK + k0 + c) : make_uint4(0u, 0u, 0u, 0u);
        }
    }
    // as they are into the store() layout: no multiply, no convert
    template <int NM>
    static __device__ __forceinline__ void store16(unsigned char* tile, int tid, const uint4 (&r)[NM]) {
        const int row0 = tid >> SH16, c = 8 * (tid & (BK / 8 - 1));
#pragma unroll
        for (int m = 0; m < NM; ++m) *(uint4*)(tile + (row0 + RP16 * m) * ROW + c * 2) = r[m];
    }
    // the entry's K tile from fp8 rows (the _rows8 entry points): load16's geometry, this thread's NM vectors
    // of 8 e4m3 bytes (a row is 768 B, so every vector is 8-B aligned), zeros past n.  A thread's rows are the
    // same in every K tile, so their scales are loaded once per block tile (load8_scale, under the same guard)
    template <int NM>
    static __device__ __forceinline__ void load8(rows8_t base, int n, int row_base, int k0, int tid, uint2 (&r)[NM]) {
        const int row0 = row_base + (tid >> SH16), c = 8 * (tid & (BK / 8 - 1));
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const int row = row0 + RP16 * m;
            r[m] = row < n ? *(const uint2*)(base.y + (long)row * CK + k0 + c) : make_uint2(0u, 0u);
        }
    }
    template <int NM>
    static __device__ __forceinline__ void load8_scale(rows8_t base, int n, int row_base, int tid, float (&s)[NM]) {
        const int row0 = row_base + (tid >> SH16);
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const int row = row0 + RP16 * m;
            s[m] = row < n ? base.s[row] : 0.f;
        }
    }
    // e4m3 -> fp32 (the hardware conversion), times the row's power of two, to bf16, into the store() layout.
    // Exact at every step: four significant bits, and the quantiser's exponent range keeps the product inside
    // bf16's normal range, so the bits are those of bf16(float(y8) * s8) whatever the rounding mode
    template <int NM>
    static __device__ __forceinline__ void store8(unsigned char* tile, int tid, const uint2 (&r)[NM],
                                                  const float (&s)[NM]) {
        const int row0 = tid >> SH16, c = 8 * (tid & (BK / 8 - 1));
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[m].x, false);
            const auto b = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[m].x, true);
            const auto d = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[m].y, false);
            const auto e = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[m].y, true);
            uint4 o;
            o.x = fpm::f2bf2(__fmul_rn(a[0], s[m]), __fmul_rn(a[1], s[m]));
            o.y = fpm::f2bf2(__fmul_rn(b[0], s[m]), __fmul_rn(b[1], s[m]));
            o.z = fpm::f2bf2(__fmul_rn(d[0], s[m]), __fmul_rn(d[1], s[m]));
            o.w = fpm::f2bf2(__fmul_rn(e[0], s[m]), __fmul_rn(e[1], s[m]));
            *(uint4*)(tile + (row0 + RP16 * m) * ROW + c * 2) = o;
        }
    }
};
}  // namespace coarse
}  // namespace fpm

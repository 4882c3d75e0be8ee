// Ragged row pack of an enrolment sub-batch (the inverse shape of rows_fetch_kernel): the padded
// SplineConv output rows of B graphs, graph b at source rows [b * nmax, b * nmax + n[b]), packed one
// after the other into the index, graph b at rows [out_off[b], out_off[b + 1]): unchanged into out32
// (fp32), rounded to bf16 into out16 (fpm::f2bf, the rounding of fpm_cast_bf16), or both from one read
// of the source.  The padding rows are never read.
// A workgroup of 192 threads takes a band of PACK_BAND rows of one graph, two rows per step, each
// thread 8 channels (two 16-B loads; two 16-B fp32 stores and / or one 16-B bf16 store); the graph's
// count and offsets are read once per workgroup.  A band's loads are all issued before its first store.
#include "fpm_common.h"
#include "fpm.h"

namespace {
constexpr int PACK_BAND = 16;
constexpr int PK = 768;

template <bool F32, bool B16>
__global__ __launch_bounds__(192) void rows_pack_kernel(const float* __restrict__ src, long src_rows,
                                                        const int* __restrict__ n, int B, int nmax,
                                                        const long* __restrict__ out_off, float* __restrict__ out32,
                                                        bf16_t* __restrict__ out16, long out_rows) {
    const int b = blockIdx.y;
    if (b >= B) return;
    const long ng = n[b];
    const long r0 = (long)b * nmax;
    const long o0 = out_off[b], no = out_off[b + 1] - o0;
    // the wrapper checks all of it on the host; never read outside src, never write outside the outputs
    if (ng < 0 || ng > nmax || no != ng || r0 + ng > src_rows || o0 < 0 || o0 + ng > out_rows) return;
    const int sub = threadIdx.x >= 96 ? 1 : 0;         // which of the step's two rows
    const int c0 = 8 * (threadIdx.x - 96 * sub);       // this thread's 8 channels
    const long band0 = (long)blockIdx.x * PACK_BAND + sub;
    float4 a[PACK_BAND / 2], c[PACK_BAND / 2];
#pragma unroll
    for (int s = 0; s < PACK_BAND / 2; ++s) {
        const long r = band0 + 2 * s;
        a[s] = c[s] = make_float4(0.f, 0.f, 0.f, 0.f);    // every element defined: the band stays in registers
        if (r < ng) {
            const float* p = src + (r0 + r) * PK + c0;
            a[s] = *(const float4*)p;
            c[s] = *(const float4*)(p + 4);
        }
    }
#pragma unroll
    for (int s = 0; s < PACK_BAND / 2; ++s) {
        const long r = band0 + 2 * s;
        if (r < ng) {
            const long o = (o0 + r) * PK + c0;
            if (F32) {
                *(float4*)(out32 + o) = a[s];
                *(float4*)(out32 + o + 4) = c[s];
            }
            if (B16) {
                uint4 h;
                h.x = (uint32_t)fpm::f2bf(a[s].x) | ((uint32_t)fpm::f2bf(a[s].y) << 16);
                h.y = (uint32_t)fpm::f2bf(a[s].z) | ((uint32_t)fpm::f2bf(a[s].w) << 16);
                h.z = (uint32_t)fpm::f2bf(c[s].x) | ((uint32_t)fpm::f2bf(c[s].y) << 16);
                h.w = (uint32_t)fpm::f2bf(c[s].z) | ((uint32_t)fpm::f2bf(c[s].w) << 16);
                *(uint4*)(out16 + o) = h;
            }
        }
    }
}
}  // namespace

extern "C" int fpm_rows_pack(const float* src, long src_rows, const int* n, int B, int nmax, const long* out_off,
                             float* out32, void* out16, long out_rows, void* stream) {
    FPM_CHECK_ARG(B >= 0 && B <= 65535 && nmax >= 0 && src_rows >= 0 && out_rows >= 0,
                  "rows_pack: bad sizes (B %d, nmax %d, src_rows %ld, out_rows %ld)", B, nmax, src_rows, out_rows);
    FPM_CHECK_ARG((long)B * nmax <= src_rows, "rows_pack: src holds %ld rows, %d graphs of %d padded rows need %ld",
                  src_rows, B, nmax, (long)B * nmax);
    FPM_CHECK_ARG(src && n && out_off, "rows_pack: src, n and out_off are required");
    FPM_CHECK_ARG(out32 || out16, "rows_pack: out32, out16 or both are required");
    FPM_CHECK_ARG((((uintptr_t)src | (uintptr_t)out32 | (uintptr_t)out16) & 15) == 0,
                  "rows_pack: src, out32 and out16 must be 16-byte aligned");
    if (B == 0 || nmax == 0) return 0;
    dim3 grid((unsigned)((nmax + PACK_BAND - 1) / PACK_BAND), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (out32 && out16)
        hipLaunchKernelGGL((rows_pack_kernel<true, true>), grid, dim3(192), 0, st, src, src_rows, n, B, nmax, out_off,
                           out32, (bf16_t*)out16, out_rows);
    else if (out32)
        hipLaunchKernelGGL((rows_pack_kernel<true, false>), grid, dim3(192), 0, st, src, src_rows, n, B, nmax, out_off,
                           out32, (bf16_t*)nullptr, out_rows);
    else
        hipLaunchKernelGGL((rows_pack_kernel<false, true>), grid, dim3(192), 0, st, src, src_rows, n, B, nmax, out_off,
                           (float*)nullptr, (bf16_t*)out16, out_rows);
    return fpm::check_launch("fpm_rows_pack");
}

// Ragged segment copy of index rows (compaction of a mutable gallery index: the rows of the live entries
// moved towards the front of their storage, or to and from a staging buffer): K segments in one launch,
// segment k from source rows [src_off[k], src_off[k] + cnt[k]) to destination rows
// [dst_off[k], dst_off[k] + cnt[k]) -- the fp32 rows (src32 -> dst32), their bf16 copy (src16 -> dst16, the
// bits as they are: nothing is rounded), or both from one table of offsets.
// Source and destination may be one buffer: the caller (ops.rows_move) then guarantees that no destination
// range meets a source range, so the order in which the workgroups run does not matter; the pointers are
// not marked restrict.
// The shape of rows_fetch_kernel and rows_pack_kernel: a workgroup of 192 threads takes a band of MOVE_BAND
// rows of one segment, two rows per step, each thread 8 channels (two 16-B fp32 loads and stores and / or
// one 16-B bf16 load and store); the segment's three numbers are read once per workgroup.  A band's loads
// are all issued before its first store.
#include "fpm_common.h"
#include "fpm.h"

namespace {
constexpr int MOVE_BAND = 16;
constexpr int MK = 768;

template <bool F32, bool B16>
__global__ __launch_bounds__(192) void rows_move_kernel(const float* src32, const bf16_t* src16, long src_rows,
                                                        const long* __restrict__ src_off,
                                                        const long* __restrict__ dst_off,
                                                        const long* __restrict__ cnt, int K, float* dst32,
                                                        bf16_t* dst16, long dst_rows) {
    const int k = blockIdx.y;
    if (k >= K) return;
    const long s0 = src_off[k], d0 = dst_off[k], nr = cnt[k];
    // the wrapper checks all of it on the host; never read outside the source, never write outside the
    // destination (the comparisons cannot overflow: nr <= src_rows and nr <= dst_rows come first)
    if (nr <= 0 || s0 < 0 || d0 < 0 || nr > src_rows || nr > dst_rows || s0 > src_rows - nr || d0 > dst_rows - nr)
        return;
    const int sub = threadIdx.x >= 96 ? 1 : 0;         // which of the step's two rows
    const int c0 = 8 * (threadIdx.x - 96 * sub);       // this thread's 8 channels
    const long band0 = (long)blockIdx.x * MOVE_BAND + sub;
    float4 a[MOVE_BAND / 2], c[MOVE_BAND / 2];
    uint4 h[MOVE_BAND / 2];
#pragma unroll
    for (int s = 0; s < MOVE_BAND / 2; ++s) {
        const long r = band0 + 2 * s;
        a[s] = c[s] = make_float4(0.f, 0.f, 0.f, 0.f);    // every element defined: the band stays in registers
        h[s] = make_uint4(0u, 0u, 0u, 0u);
        if (r < nr) {
            const long o = (s0 + r) * MK + c0;
            if (F32) {
                a[s] = *(const float4*)(src32 + o);
                c[s] = *(const float4*)(src32 + o + 4);
            }
            if (B16) h[s] = *(const uint4*)(src16 + o);
        }
    }
#pragma unroll
    for (int s = 0; s < MOVE_BAND / 2; ++s) {
        const long r = band0 + 2 * s;
        if (r < nr) {
            const long o = (d0 + r) * MK + c0;
            if (F32) {
                *(float4*)(dst32 + o) = a[s];
                *(float4*)(dst32 + o + 4) = c[s];
            }
            if (B16) *(uint4*)(dst16 + o) = h[s];
        }
    }
}
}  // namespace

extern "C" int fpm_rows_move(const float* src32, const void* src16, long src_rows, const long* src_off,
                             const long* dst_off, const long* cnt, int K, int band_rows, float* dst32, void* dst16,
                             long dst_rows, void* stream) {
    FPM_CHECK_ARG(K >= 0 && K <= 65535 && band_rows >= 0 && src_rows >= 0 && dst_rows >= 0,
                  "rows_move: bad sizes (K %d, band_rows %d, src_rows %ld, dst_rows %ld)", K, band_rows, src_rows,
                  dst_rows);
    FPM_CHECK_ARG(src_off && dst_off && cnt, "rows_move: src_off, dst_off and cnt are required");
    FPM_CHECK_ARG((src32 != nullptr) == (dst32 != nullptr) && (src16 != nullptr) == (dst16 != nullptr),
                  "rows_move: src32 goes with dst32, src16 with dst16");
    FPM_CHECK_ARG(src32 || src16, "rows_move: the fp32 rows, the bf16 rows or both are required");
    FPM_CHECK_ARG((((uintptr_t)src32 | (uintptr_t)src16 | (uintptr_t)dst32 | (uintptr_t)dst16) & 15) == 0,
                  "rows_move: the rows must be 16-byte aligned");
    if (K == 0 || band_rows == 0) return 0;
    dim3 grid((unsigned)((band_rows + MOVE_BAND - 1) / MOVE_BAND), (unsigned)K);
    hipStream_t st = (hipStream_t)stream;
    if (src32 && src16)
        hipLaunchKernelGGL((rows_move_kernel<true, true>), grid, dim3(192), 0, st, src32, (const bf16_t*)src16,
                           src_rows, src_off, dst_off, cnt, K, dst32, (bf16_t*)dst16, dst_rows);
    else if (src32)
        hipLaunchKernelGGL((rows_move_kernel<true, false>), grid, dim3(192), 0, st, src32, (const bf16_t*)nullptr,
                           src_rows, src_off, dst_off, cnt, K, dst32, (bf16_t*)nullptr, dst_rows);
    else
        hipLaunchKernelGGL((rows_move_kernel<false, true>), grid, dim3(192), 0, st, (const float*)nullptr,
                           (const bf16_t*)src16, src_rows, src_off, dst_off, cnt, K, (float*)nullptr, (bf16_t*)dst16,
                           dst_rows);
    return fpm::check_launch("fpm_rows_move");
}

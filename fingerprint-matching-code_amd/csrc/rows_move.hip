// Ragged segment copy of index rows (compaction of a mutable gallery index: the rows of the live entries
// moved towards the front of their storage, or to and from a staging buffer): K segments in one launch,
// segment k from source rows [src_off[k], src_off[k] + cnt[k]) to destination rows
// [dst_off[k], dst_off[k] + cnt[k]) -- the fp32 rows (src32 -> dst32), their bf16 copy (src16 -> dst16, the
// bits as they are: nothing is rounded), or both from one table of offsets; or (fpm_rows_move8) the e4m3 rows of
// an fp8 index with their fp32 row scales (src8 / srcs -> dst8 / dsts), the same kernel over that row type.
// Source and destination may be one buffer: the caller (ops.rows_move) then guarantees that no destination
// range meets a source range, so the order in which the workgroups run does not matter; the pointers are
// not marked restrict.
// The shape of rows_fetch_kernel and rows_pack_kernel: a workgroup of 192 threads takes a band of MOVE_BAND
// rows of one segment, two rows per step, each thread 8 channels (two 16-B fp32 loads and stores and / or
// one 16-B bf16 load and store, or one 8-B e4m3 load and store, the row's first thread its scale too); the
// segment's three numbers are read once per workgroup.  A band's loads are all issued before its first store.
#include "fpm_common.h"
#include "fpm.h"

namespace {
constexpr int MOVE_BAND = 16;
constexpr int MK = 768;

// the rows of one launch: fp32 and / or bf16 rows (F32, B16), or e4m3 rows with their scales (B8)
struct MoveRows {
    const float* src32;
    const bf16_t* src16;
    const unsigned char* src8;
    const float* srcs;
    float* dst32;
    bf16_t* dst16;
    unsigned char* dst8;
    float* dsts;
};

template <bool F32, bool B16, bool B8>
__global__ __launch_bounds__(192) void rows_move_kernel(MoveRows rw, long src_rows, const long* __restrict__ src_off,
                                                        const long* __restrict__ dst_off,
                                                        const long* __restrict__ cnt, int K, long dst_rows) {
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
    uint2 q[MOVE_BAND / 2];
    float sc[MOVE_BAND / 2];
#pragma unroll
    for (int s = 0; s < MOVE_BAND / 2; ++s) {
        const long r = band0 + 2 * s;
        a[s] = c[s] = make_float4(0.f, 0.f, 0.f, 0.f);    // every element defined: the band stays in registers
        h[s] = make_uint4(0u, 0u, 0u, 0u);
        q[s] = make_uint2(0u, 0u);
        sc[s] = 0.f;
        if (r < nr) {
            const long o = (s0 + r) * MK + c0;
            if (F32) {
                a[s] = *(const float4*)(rw.src32 + o);
                c[s] = *(const float4*)(rw.src32 + o + 4);
            }
            if (B16) h[s] = *(const uint4*)(rw.src16 + o);
            if (B8) {
                q[s] = *(const uint2*)(rw.src8 + o);
                if (c0 == 0) sc[s] = rw.srcs[s0 + r];
            }
        }
    }
#pragma unroll
    for (int s = 0; s < MOVE_BAND / 2; ++s) {
        const long r = band0 + 2 * s;
        if (r < nr) {
            const long o = (d0 + r) * MK + c0;
            if (F32) {
                *(float4*)(rw.dst32 + o) = a[s];
                *(float4*)(rw.dst32 + o + 4) = c[s];
            }
            if (B16) *(uint4*)(rw.dst16 + o) = h[s];
            if (B8) {
                *(uint2*)(rw.dst8 + o) = q[s];
                if (c0 == 0) rw.dsts[d0 + r] = sc[s];
            }
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
    const MoveRows rw{src32, (const bf16_t*)src16, nullptr, nullptr, dst32, (bf16_t*)dst16, nullptr, nullptr};
    if (src32 && src16)
        hipLaunchKernelGGL((rows_move_kernel<true, true, false>), grid, dim3(192), 0, st, rw, src_rows, src_off, dst_off,
                           cnt, K, dst_rows);
    else if (src32)
        hipLaunchKernelGGL((rows_move_kernel<true, false, false>), grid, dim3(192), 0, st, rw, src_rows, src_off,
                           dst_off, cnt, K, dst_rows);
    else
        hipLaunchKernelGGL((rows_move_kernel<false, true, false>), grid, dim3(192), 0, st, rw, src_rows, src_off,
                           dst_off, cnt, K, dst_rows);
    return fpm::check_launch("fpm_rows_move");
}

extern "C" int fpm_rows_move8(const void* src8, const float* srcs, long src_rows, const long* src_off,
                              const long* dst_off, const long* cnt, int K, int band_rows, void* dst8, float* dsts,
                              long dst_rows, void* stream) {
    FPM_CHECK_ARG(K >= 0 && K <= 65535 && band_rows >= 0 && src_rows >= 0 && dst_rows >= 0,
                  "rows_move8: bad sizes (K %d, band_rows %d, src_rows %ld, dst_rows %ld)", K, band_rows, src_rows,
                  dst_rows);
    FPM_CHECK_ARG(src_off && dst_off && cnt, "rows_move8: src_off, dst_off and cnt are required");
    FPM_CHECK_ARG(src8 && srcs && dst8 && dsts, "rows_move8: the e4m3 rows and their scales, source and destination, "
                                                "are required");
    FPM_CHECK_ARG((((uintptr_t)src8 | (uintptr_t)dst8) & 15) == 0 && (((uintptr_t)srcs | (uintptr_t)dsts) & 3) == 0,
                  "rows_move8: the rows must be 16-byte aligned, the scales 4-byte aligned");
    if (K == 0 || band_rows == 0) return 0;
    dim3 grid((unsigned)((band_rows + MOVE_BAND - 1) / MOVE_BAND), (unsigned)K);
    const MoveRows rw{nullptr, nullptr, (const unsigned char*)src8, srcs, nullptr, nullptr, (unsigned char*)dst8, dsts};
    hipLaunchKernelGGL((rows_move_kernel<false, false, true>), grid, dim3(192), 0, (hipStream_t)stream, rw, src_rows,
                       src_off, dst_off, cnt, K, dst_rows);
    return fpm::check_launch("fpm_rows_move8");
}

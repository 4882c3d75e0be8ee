// Ragged row copy of an enrolled gallery (1:N identification over an index whose fp32 rows live in
// pinned host memory): the rows of the M selected entries, entry idx[m] at source rows
// [row_off[idx[m]], row_off[idx[m] + 1]), packed one after the other into a device staging buffer,
// entry m at rows [out_off[m], out_off[m + 1]).  The source is any device-readable fp32 memory: a
// device tensor, or a pinned host tensor read through its device mapping (the kernel then is the
// host-to-device transfer, one launch for the whole ragged selection).
// The shape of rows_gather_scale_kernel: a workgroup of 192 threads takes a band of FETCH_BAND rows
// of one entry, two rows per step, each thread 8 channels (two 16-B loads, two 16-B stores); the
// entry's offsets are read once per workgroup.  A band's loads are all issued before its first store,
// so a thread keeps 256 B in flight on the way from the host.
#include "fpm_common.h"
#include "fpm.h"

namespace {
constexpr int FETCH_BAND = 16;
constexpr int FK = 768;

__global__ __launch_bounds__(192) void rows_fetch_kernel(const float* __restrict__ src, long src_rows,
                                                         const long* __restrict__ row_off,
                                                         const int* __restrict__ idx, int G,
                                                         float* __restrict__ out, long out_rows,
                                                         const long* __restrict__ out_off) {
    const int m = blockIdx.y;
    const int g = idx[m];
    if (g < 0 || g >= G) return;                       // the wrapper checks the range; never read outside src
    const long r0 = row_off[g], ng = row_off[g + 1] - r0;
    const long o0 = out_off[m], no = out_off[m + 1] - o0;
    // the wrapper checks all of it on the host; never read outside src, never write outside out
    if (ng < 0 || no != ng || r0 < 0 || r0 + ng > src_rows || o0 < 0 || o0 + ng > out_rows) return;
    const int sub = threadIdx.x >= 96 ? 1 : 0;         // which of the step's two rows
    const int c0 = 8 * (threadIdx.x - 96 * sub);       // this thread's 8 channels
    const long band0 = (long)blockIdx.x * FETCH_BAND + sub;
    float4 a[FETCH_BAND / 2], c[FETCH_BAND / 2];
#pragma unroll
    for (int s = 0; s < FETCH_BAND / 2; ++s) {
        const long r = band0 + 2 * s;
        if (r < ng) {
            const float* p = src + (r0 + r) * FK + c0;
            a[s] = *(const float4*)p;
            c[s] = *(const float4*)(p + 4);
        }
    }
#pragma unroll
    for (int s = 0; s < FETCH_BAND / 2; ++s) {
        const long r = band0 + 2 * s;
        if (r < ng) {
            float* p = out + (o0 + r) * FK + c0;
            *(float4*)p = a[s];
            *(float4*)(p + 4) = c[s];
        }
    }
}
}  // namespace

extern "C" int fpm_rows_fetch(const float* src, long src_rows, const long* row_off, const int* idx, int G, int M,
                              int nmax, float* out, long out_rows, const long* out_off, void* stream) {
    FPM_CHECK_ARG(G > 0 && M >= 0 && M <= 65535 && nmax >= 0 && src_rows >= 0 && out_rows >= 0,
                  "rows_fetch: bad sizes (G %d, M %d, nmax %d, src_rows %ld, out_rows %ld)", G, M, nmax, src_rows,
                  out_rows);
    FPM_CHECK_ARG(src && row_off && idx && out && out_off, "rows_fetch: src, row_off, idx, out and out_off are required");
    FPM_CHECK_ARG((((uintptr_t)src | (uintptr_t)out) & 15) == 0, "rows_fetch: src and out must be 16-byte aligned");
    if (M == 0 || nmax == 0) return 0;
    dim3 grid((unsigned)((nmax + FETCH_BAND - 1) / FETCH_BAND), (unsigned)M);
    hipLaunchKernelGGL(rows_fetch_kernel, grid, dim3(192), 0, (hipStream_t)stream, src, src_rows, row_off, idx, G, out,
                       out_rows, out_off);
    return fpm::check_launch("fpm_rows_fetch");
}

// Micro-benchmark of the SplineConv product GEMM shapes: 128x128 register-staged kernel
// (gemm_core.h), the 256x256 LDS-DMA kernels (gemm_big.h, gemm_phase.h) and the strip walk
// (gemm_walk_kernel, strips of two row tiles per workgroup); checks the outputs are identical.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I fingerprint-matching-code_amd/csrc tools/gemm_bench.hip
// (-DGP_PROBE: also the per-workgroup phase split of the phase and walk kernels from shader-clock stamps)
//   gemm_bench [nodes N]            grouped SplineConv shape over N nodes (default 32768, ~9.7 rows per node)
//   gemm_bench dense M N K [M N K]  dense GEMMs, no gather, no groups
#include "gemm_phase.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <random>
#include <algorithm>
#include <cstring>

namespace fpm {
int& gemm_walk_flag() { static int v = GW_AUTO; return v; }
int gemm_cu_count() { return 256; }
void set_error(const char*, ...) {}
int check_launch(const char*) { return 0; }
}
using namespace fpm;

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

static uint16_t h_f2bf(float f) { uint32_t u; memcpy(&u, &f, 4); u += 0x7FFF + ((u >> 16) & 1); return (uint16_t)(u >> 16); }

// variant v of the 256-row kernels: 0 two-stage, 1 phase, 2 walk with strips of 2 forced, 3 walk
// under the rule, 4 phase with the direct-from-register epilogue
constexpr int NV = 5;
static const char* vname(int v) {
    static const char* n[] = {"256x256", "phase256", "walk S=2", "walk rule", "direct256"};
    return n[v];
}
static unsigned walk_grid(const GemmParams& p) {   // an upper bound of gemm_walk_launch's grid
    return (unsigned)((p.remap_mtiles + 7) / 8 * 8 * (p.N / 256));
}
static void launch256(int v, const GemmParams& p) {
    if (v == 0) hipLaunchKernelGGL((gemm_big_kernel<256, EPI_STORE, false>), dim3(remap_grid256(p.N, p.remap_mtiles)), dim3(G2_THREADS), 0, 0, p);
    else if (v == 1) hipLaunchKernelGGL((gemm_phase_kernel<EPI_STORE, false>), dim3(remap_grid256(p.N, p.remap_mtiles)), dim3(G2_THREADS), 0, 0, p);
    else if (v == 4) hipLaunchKernelGGL((gemm_phase_kernel<EPI_STORE, false, true>), dim3(remap_grid256(p.N, p.remap_mtiles)), dim3(G2_THREADS), 0, 0, p);
    else gemm_walk_launch(p, v == 2 ? 2 : GW_AUTO, 1, 0);
}

// dense C[M][N] = A[M][K] . B[N][K]^T with the 256x256 kernels (no gather, no groups)
static int dense(int M, int N, int K) {
    std::mt19937 rng(2);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    std::vector<uint16_t> ha((size_t)M * K), hb((size_t)N * K);
    for (auto& v : ha) v = h_f2bf(U(rng));
    for (auto& v : hb) v = h_f2bf(U(rng));
    uint16_t *da, *db, *c[NV];
    CK(hipMalloc(&da, ha.size() * 2)); CK(hipMalloc(&db, hb.size() * 2));
    for (auto& x : c) { CK(hipMalloc(&x, (size_t)M * N * 2)); CK(hipMemset(x, 0, (size_t)M * N * 2)); }
    CK(hipMemcpy(da, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(db, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
    GemmParams p = {};
    p.A = da; p.lda = K; p.B = db; p.ldb = K; p.M = M; p.N = N; p.K = K; p.nseg = 1; p.epi = EPI_STORE; p.ldc = N;
    p.remap_mtiles = (M + 255) / 256;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const double flops = 2.0 * M * (double)N * K;
    for (int round = 0; round < 3; ++round)
        for (int v = 0; v < NV; ++v) {
            GemmParams pv = p; pv.Ct = c[v];
            CK(hipEventRecord(e0));
            for (int r = 0; r < 10; ++r) launch256(v, pv);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            ms /= 10;
            printf("dense %dx%dx%d round %d %-9s %.4f ms  %.1f TF/s\n", M, N, K, round, vname(v), ms, flops / ms / 1e9);
        }
    std::vector<uint16_t> h0((size_t)M * N), hv((size_t)M * N);
    CK(hipMemcpy(h0.data(), c[0], h0.size() * 2, hipMemcpyDeviceToHost));
    size_t bad = 0;
    for (int v = 1; v < NV; ++v) {
        CK(hipMemcpy(hv.data(), c[v], hv.size() * 2, hipMemcpyDeviceToHost));
        size_t diff = 0;
        for (size_t i = 0; i < h0.size(); ++i) diff += h0[i] != hv[i];
        printf("dense %dx%dx%d mismatching elements %s vs 256x256: %zu of %zu\n", M, N, K, vname(v), diff, h0.size());
        bad += diff;
    }
    CK(hipFree(da)); CK(hipFree(db));
    for (auto x : c) CK(hipFree(x));
    return bad != 0;
}

#ifdef GP_PROBE
static std::vector<unsigned long long> probe_run(int v, const GemmParams& p, size_t nwg) {
    unsigned long long* d;
    CK(hipMalloc(&d, nwg * 8 * sizeof(unsigned long long)));
    CK(hipMemset(d, 0, nwg * 8 * sizeof(unsigned long long)));
    CK(hipMemcpyToSymbol(HIP_SYMBOL(gp_probe_buf), &d, sizeof(d)));
    launch256(v, p);
    CK(hipDeviceSynchronize());
    std::vector<unsigned long long> h(nwg * 8);
    CK(hipMemcpy(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost));
    unsigned long long* none = nullptr;
    CK(hipMemcpyToSymbol(HIP_SYMBOL(gp_probe_buf), &none, sizeof(none)));
    CK(hipFree(d));
    return h;
}
// per-workgroup phase split of one phase-kernel launch from the GP_STAMP shader-clock stamps
static void probe_report(const GemmParams& p) {
    const size_t nwg = remap_grid256(p.N, p.remap_mtiles);
    const auto h = probe_run(1, p, nwg);
    double sum[6] = {0, 0, 0, 0, 0, 0}, life = 0;
    unsigned long long tmin = ~0ull, tmax = 0;
    long n = 0;
    for (size_t w = 0; w < nwg; ++w) {
        const unsigned long long* t = &h[w * 8];
        if (!t[0] || !t[5]) continue;
        for (int k = 1; k < 6; ++k) sum[k] += (double)(t[k] - t[k - 1]);
        life += (double)(t[5] - t[0]);
        tmin = std::min(tmin, t[0]);
        tmax = std::max(tmax, t[5]);
        ++n;
    }
    printf("probe phase256: %ld workgroups; mean clocks per workgroup: prologue %.0f, main loop %.0f, epilogue image %.0f, "
           "store issue %.0f, store retire %.0f, lifetime %.0f; span %llu clocks; sum of lifetimes / (span x 256) = %.3f\n",
           n, sum[1] / n, sum[2] / n, sum[3] / n, sum[4] / n, sum[5] / n, life / n, tmax - tmin, life / ((double)(tmax - tmin) * 256));
}
// the walk's stamps (first tile of each strip of two): per-tile split
static void probe_report_walk(const GemmParams& p) {
    const int S = 2;
    const size_t nwg = walk_grid(p);
    const auto h = probe_run(2, p, nwg);
    double loop = 0, lead = 0, epi = 0, drain = 0, tile = 0;
    long n = 0;
    for (size_t w = 0; w < nwg; ++w) {
        const unsigned long long* t = &h[w * 8];
        if (!t[0] || !t[1] || !t[4]) continue;
        loop += (double)(t[2] - t[0]); lead += (double)(t[2] - t[1]); epi += (double)(t[3] - t[2]);
        drain += (double)(t[4] - t[3]); tile += (double)(t[4] - t[0]);
        ++n;
    }
    if (!n) { printf("probe walk S=%d: no strip with a stamped tile\n", S); return; }
    printf("probe walk S=%d: %ld stamped tiles; mean clocks per tile: main loop %.0f (next tile's first DMA issued %.0f before "
           "its end), image + stores %.0f, boundary drain (next tile's first K-tile landed) %.0f, tile %.0f\n",
           S, n, loop / n, lead / n, epi / n, drain / n, tile / n);
}
#endif

int main(int argc, char** argv) {
#ifdef GP_PROBE
    {   // stamps stay off (null buffer) outside the probe runs
        unsigned long long* none = nullptr;
        CK(hipMemcpyToSymbol(HIP_SYMBOL(gp_probe_buf), &none, sizeof(none)));
    }
#endif
    if (argc > 1 && !strcmp(argv[1], "dense")) {
        int rc = 0;
        for (int i = 2; i + 2 <= argc - 1; i += 3) rc |= dense(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]));
        return rc;
    }
    const int Nn = argc > 2 && !strcmp(argv[1], "nodes") ? atoi(argv[2]) : 32768, D = 768, NC = 26;
    std::mt19937 rng(1);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    std::vector<uint16_t> hx((size_t)Nn * D), hw((size_t)NC * D * D);
    for (auto& v : hx) v = h_f2bf(U(rng));
    for (auto& v : hw) v = h_f2bf(U(rng) * 0.05f);
    // cell row sets: 9 dense cells (~97% of nodes), 8 sparse cells, root = all nodes
    std::vector<int> arows, goff(NC + 1);
    std::uniform_real_distribution<float> P(0.f, 1.f);
    for (int c = 0; c < NC; ++c) {
        goff[c] = (int)arows.size();
        float pr = c == 25 ? 1.f : ((c % 5 >= 1 && c % 5 <= 3 && c / 5 >= 1 && c / 5 <= 3) ? 0.97f : 0.002f);
        for (int u = 0; u < Nn; ++u) if (P(rng) < pr) arows.push_back(u);
    }
    goff[NC] = (int)arows.size();
    const int rows = goff[NC];
    auto table = [&](int tb) {
        std::vector<int> t;
        for (int c = 0; c < NC; ++c)
            for (int r = goff[c]; r < goff[c + 1]; r += tb) { t.push_back(c); t.push_back(r); }
        int real = (int)t.size() / 2;
        int maxt = rows / tb + NC + 1;
        for (int i = real; i < maxt; ++i) { t.push_back(-1); t.push_back(0); }
        return t;
    };
    auto t128 = table(128), t256 = table(256);
    printf("nodes %d rows %d  tiles128 %zu tiles256 %zu\n", Nn, rows, t128.size() / 2, t256.size() / 2);
    uint16_t *dx, *dw, *c1, *cv[NV];
    int *darows, *dgoff, *dt128, *dt256, *dtc;
    CK(hipMalloc(&dx, hx.size() * 2)); CK(hipMalloc(&dw, hw.size() * 2));
    CK(hipMalloc(&c1, (size_t)rows * D * 2));
    for (auto& x : cv) { CK(hipMalloc(&x, (size_t)rows * D * 2)); CK(hipMemset(x, 0, (size_t)rows * D * 2)); }
    CK(hipMalloc(&darows, arows.size() * 4)); CK(hipMalloc(&dgoff, goff.size() * 4));
    CK(hipMalloc(&dt128, t128.size() * 4)); CK(hipMalloc(&dt256, t256.size() * 4));
    CK(hipMemcpy(dx, hx.data(), hx.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(dw, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(darows, arows.data(), arows.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dgoff, goff.data(), goff.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dt128, t128.data(), t128.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dt256, t256.data(), t256.size() * 4, hipMemcpyHostToDevice));
    GemmParams p = {};
    p.A = dx; p.lda = D; p.a_rows = darows; p.B = dw; p.ldb = D; p.sB_seg = (long)D * D;
    p.M = rows; p.N = D; p.K = D; p.nseg = 1; p.group_off = dgoff; p.epi = EPI_STORE; p.ldc = D;
    GemmParams p1 = p, p2 = p;
    p1.tile_info = dt128; p1.Ct = c1; p1.remap_mtiles = (int)t128.size() / 2;
    p2.tile_info = dt256; p2.remap_mtiles = (int)t256.size() / 2;
    int real256 = 0;
    for (size_t i = 0; i < t256.size(); i += 2) real256 += t256[i] >= 0;
    CK(hipMalloc(&dtc, 4)); CK(hipMemcpy(dtc, &real256, 4, hipMemcpyHostToDevice));
    p2.tile_count = dtc;
    printf("real 256-row tiles %d; the rule's strip length for this launch: %d\n", real256,
           p2.remap_mtiles * 3L >= 8L * gemm_cu_count() ? 2 : gemm_walk_rule(real256, D / 256, gemm_cu_count()));
    dim3 g1(remap_grid(D, p1.remap_mtiles));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const double flops = 2.0 * rows * (double)D * D;
    const int reps = 20;
    for (int round = 0; round < 4; ++round) {
        for (int v = -1; v < NV; ++v) {
            if (v == -1 && round > 0) continue;
            GemmParams pv = p2;
            if (v >= 0) pv.Ct = cv[v];
            CK(hipEventRecord(e0));
            for (int r = 0; r < reps; ++r) {
                if (v == -1) hipLaunchKernelGGL((gemm_kernel<bf16_t, false>), g1, dim3(GTHREADS), 0, 0, p1);
                else launch256(v, pv);
            }
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            ms /= reps;
            printf("round %d %-10s %.4f ms  %.1f TF/s\n", round, v < 0 ? "128x128" : vname(v), ms, flops / ms / 1e9);
        }
    }
    // tile order: row tiles per XCD chunk (remap_cm), phase kernel
    for (int round = 0; round < 2; ++round)
        for (int cm : {1, 2, 4, 8, 16}) {
            GemmParams pc = p2; pc.Ct = cv[1]; pc.remap_cm = cm;
            dim3 gc(remap_grid_big(D, 256, pc.remap_mtiles, cm));
            CK(hipEventRecord(e0));
            for (int r = 0; r < reps; ++r) hipLaunchKernelGGL((gemm_phase_kernel<EPI_STORE, false>), gc, dim3(G2_THREADS), 0, 0, pc);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            ms /= reps;
            printf("round %d phase256 chunk %2d m-tiles %.4f ms  %.1f TF/s\n", round, cm, ms, flops / ms / 1e9);
        }
#ifdef GP_PROBE
    {
        GemmParams pp = p2; pp.Ct = cv[1];
        for (int r = 0; r < 2; ++r) probe_report(pp);
        pp.Ct = cv[2];
        for (int r = 0; r < 2; ++r) probe_report_walk(pp);
    }
#endif
    std::vector<uint16_t> h1((size_t)rows * D), h0((size_t)rows * D), hv((size_t)rows * D);
    CK(hipMemcpy(h1.data(), c1, h1.size() * 2, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h0.data(), cv[0], h0.size() * 2, hipMemcpyDeviceToHost));
    size_t bad = 0;
    for (size_t i = 0; i < h1.size(); ++i) bad += h1[i] != h0[i];
    printf("mismatching elements 128 vs 256: %zu of %zu\n", bad, h1.size());
    for (int v = 1; v < NV; ++v) {
        CK(hipMemcpy(hv.data(), cv[v], hv.size() * 2, hipMemcpyDeviceToHost));
        size_t diff = 0;
        for (size_t i = 0; i < h0.size(); ++i) diff += hv[i] != h0[i];
        printf("mismatching elements %s vs 256x256: %zu of %zu\n", vname(v), diff, h0.size());
        bad += diff;
    }
    return bad != 0;
}

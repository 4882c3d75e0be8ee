// Phase-pipelined 256 x 256 bf16 MFMA GEMM tile (the SplineConv (node, cell) product GEMM and the
// other large bf16 GEMMs with N % 256 == 0).  Same contract and results as gemm_big_kernel<256>
// (gemm_big.h): identical per-element accumulation order, so the outputs are bit-identical.
//
// Why a second kernel: gemm_big_kernel retires every K-tile's LDS-DMA with vmcnt(0) + a workgroup
// barrier, so each K-step stalls on its own prefetch (the "~900 TF" structure).  Here the K loop is
// cut into PHASES, one per C-quadrant of each wave, and the LDS-DMA stream runs 3-4 phases ahead:
//
// * 512 threads = 8 waves = 2 groups (wr) x 4 (wc).  A wave owns rows {h*128 + wr*64 + [0,64)} and
//   columns {g*128 + wc*32 + [0,32)}, h, g in {0,1}: its 128 x 64 output is four 64 x 32 quadrants
//   (h, g), each 4 x 2 16x16 fragments = 16 MFMA 16x16x32 per 64-deep K-tile.
// * LDS: two K-tile buffers, each four HALF-TILES A0, A1 (A rows h*128..+128), B0, B1 (B rows =
//   output columns g*128..+128); a half-tile is 128 rows x 128 B (BK = 64 bf16), filled by two
//   global_load_lds_dwordx4 per thread, XOR-swizzled on the source address exactly as gemm_big.h.
// * K-tile t runs phases q = 0..3 on quadrants (0,0) (0,1) (1,1) (1,0); the A fragments of half h
//   and the B fragments of both halves stay in registers across the phases that share them, so
//   each K-tile reads the 24 fragments once: q0 reads A0 + B0, q1 B1, q2 A1, q3 nothing.
// * One half-tile of LDS-DMA is issued per phase, in the order A0 B0 B1 A1 of each K-tile, six
//   half-tiles ahead of the phase stream: phase phi issues half-tile j = phi + 6 and, before that,
//   retires j = phi + 2 with s_waitcnt vmcnt(6) (2 instructions per younger half-tile).  Every
//   half-tile is retired at least one phase before its first read and re-staged at least two
//   phases after its last read (the RAW / WAR rules with the barriers below).
// * Each phase: [wait; issue; ds_reads] s_barrier, lgkmcnt(0), MFMAs at raised priority, s_barrier.
//   Group wr = 1 runs one barrier behind group 0, so on every SIMD one wave's MFMAs overlap the
//   other wave's LDS reads and DMA issue.  Raw s_barrier only: __syncthreads() would drain the
//   in-flight DMA (vmcnt(0)).  All LDS is the one __shared__ array (a second one makes the
//   compiler wait vmcnt(0) before the ds_reads).
// * The last two K-tiles are peeled with their exact vmcnt counts (no issues past the end).
#pragma once
#include <type_traits>
#include "gemm_big.h"

namespace fpm {

constexpr int GP_HALF = 128 * 128;                        // bytes per half-tile
constexpr int GP_SMEM = g2_max(8 * GP_HALF, G2_BM * (2 * 256 + 16));
constexpr int GP_MIN_KTILES = 2;

#define FPM_VMCNT(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")

// GP_PROBE (tools/gemm_bench.hip only, never in the library): per-workgroup shader-clock stamps at
// entry, main-loop start, main-loop end, epilogue image written, stores issued, stores retired
// (wave 0) -> gp_probe_buf[wg * 8 + k]
#ifdef GP_PROBE
__device__ unsigned long long* gp_probe_buf;
#define GP_STAMP(k)                                                                                   \
    do {                                                                                              \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();                                   \
        if (threadIdx.x == 0 && gp_probe_buf)                                                         \
            gp_probe_buf[((long)blockIdx.z * gridDim.x + blockIdx.x) * 8 + (k)] = t_;                   \
    } while (0)
#else
#define GP_STAMP(k)
#endif

#ifndef GP_STAGGER
#define GP_STAGGER 1
#endif
#ifndef GP_PRIO
#define GP_PRIO 1
#endif
// DIRECT (bf16 output): the MFMAs run with swapped operands (weights as the first), so each lane's
// accumulator holds 4 consecutive OUTPUT COLUMNS of one row, and the epilogue stores them straight
// from registers (8 B per lane, no LDS image, no barrier)
template <int EPI, bool F32OUT, bool DIRECT = false>
__global__ __launch_bounds__(G2_THREADS, 1) void gemm_phase_kernel(GemmParams p) {
    constexpr int BN = 256;
    __shared__ __attribute__((aligned(16))) unsigned char smem[GP_SMEM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 2, wc = wave & 3;
    const int batch = blockIdx.z;

    const int nt = (p.N + BN - 1) / BN;
    const int q = remap_tile(nt, p.remap_mtiles, p.remap_cm > 0 ? p.remap_cm : 4);
    const int mtile = q / nt, ntile = q - mtile * nt;
    if (mtile >= p.remap_mtiles) return;
    int group = 0, row0, row_end;
    if (p.tile_info) {
        group = p.tile_info[2 * mtile];
        if (group < 0) return;
        row0 = p.tile_info[2 * mtile + 1];
        row_end = p.group_off[group + 1];
    } else {
        row0 = mtile * G2_BM;
        row_end = p.M;
    }
    const int n0 = ntile * BN;
    const bf16_t* A = (const bf16_t*)p.A + (long)batch * p.sA;
    const bf16_t* Bg = (const bf16_t*)p.B + (long)batch * p.sB + (long)group * p.sB_seg;

    // DMA sources: half-tile piece i of wave w = rows 8*(2w+i) + (lane>>3) of the half,
    // K-chunk (lane&7) ^ ((row>>1)&7)
    const bf16_t* src[4][2];                              // [A0, A1, B0, B1][piece]
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (wave * 2 + i) * 8 + (lane >> 3);
        const int kc = (lane & 7) ^ ((r >> 1) & 7);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int gr = row0 + h * 128 + r;
            gr = gr < row_end ? gr : row0;                // clamp: rows past the end are never stored
            const long arow = p.a_rows ? (long)p.a_rows[gr] : (long)gr;
            src[h][i] = A + arow * p.lda + kc * 8;
            const int n = n0 + h * 128 + r < p.N ? n0 + h * 128 + r : p.N - 1;
            src[2 + h][i] = Bg + (long)n * p.ldb + kc * 8;
        }
    }
    // half-tile stream j: K-tile j >> 2, kind j & 3 in the order A0 B0 B1 A1 -> buffer slot
    auto issue = [&](int j, int slot) {
        const int t = j >> 2;
        unsigned char* dst = smem + ((t & 1) * 4 + slot) * GP_HALF + wave * 2048;
        const int k0 = t * G2_BK;
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src[slot][0] + k0), (lds_ptr_t)dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src[slot][1] + k0), (lds_ptr_t)(dst + 1024), 16, 0, 0);
    };

    // fragment reads: A half row wr*64 + f*16 + (lane&15) (f < 4), B half row wc*32 + f*16 +
    // (lane&15) (f < 2); K-chunk c = kk*4 + (lane>>4) at slot c ^ ((lane>>1)&7)
    const int xr = (lane >> 1) & 7;
    const int a_off = (wr * 64 + (lane & 15)) * 128;
    const int b_off = (wc * 32 + (lane & 15)) * 128;
    const int s0 = ((lane >> 4) ^ xr) * 16, s1 = ((4 + (lane >> 4)) ^ xr) * 16;

    f32x4_t acc[2][2][4][2];                              // [h][g][fm][fn]
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[h][g][i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    bf16x8_t a[2][4], b0[2][2], b1[2][2];                 // [kk][frag]

    auto read_a = [&](int t, int h) {
        const unsigned char* base = smem + ((t & 1) * 4 + h) * GP_HALF + a_off;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            a[0][f] = *(const bf16x8_t*)(base + f * 2048 + s0);
            a[1][f] = *(const bf16x8_t*)(base + f * 2048 + s1);
        }
    };
    auto read_b = [&](int t, int g, bf16x8_t (&bb)[2][2]) {
        const unsigned char* base = smem + ((t & 1) * 4 + 2 + g) * GP_HALF + b_off;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            bb[0][f] = *(const bf16x8_t*)(base + f * 2048 + s0);
            bb[1][f] = *(const bf16x8_t*)(base + f * 2048 + s1);
        }
    };
    auto mfma = [&](f32x4_t (&c)[4][2], bf16x8_t (&bb)[2][2]) {
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (GP_PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int fm = 0; fm < 4; ++fm)
#pragma unroll
                for (int fn = 0; fn < 2; ++fn) {
                    if constexpr (DIRECT)
                        c[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bb[kk][fn], a[kk][fm], c[fm][fn], 0, 0, 0);
                    else
                        c[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kk][fm], bb[kk][fn], c[fm][fn], 0, 0, 0);
                }
        if (GP_PRIO) __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_s_barrier();
    };
    // slots of the kinds A0 B0 B1 A1
    constexpr int SLOT[4] = {0, 2, 3, 1};
    // one K-tile = 4 phases; VMq = vmcnt before phase q's issue (-1: none), ISSq: phase q issues
    auto ktile = [&](int t, auto VM0, auto VM1, auto VM2, auto VM3, bool iss0, bool iss1, bool iss2, bool iss3) {
        const int phi = 4 * t;
        // q0: quadrant (0,0), reads A0 + B0; issues j = phi + 6 (B1 of t+1)
        if constexpr (decltype(VM0)::value == 6) FPM_VMCNT(6);
        else if constexpr (decltype(VM0)::value == 4) FPM_VMCNT(4);
        else if constexpr (decltype(VM0)::value == 2) FPM_VMCNT(2);
        else if constexpr (decltype(VM0)::value == 0) FPM_VMCNT(0);
        if (iss0) issue(phi + 6, SLOT[(0 + 6) & 3]);
        read_a(t, 0);
        read_b(t, 0, b0);
        mfma(acc[0][0], b0);
        // q1: quadrant (0,1), reads B1; issues A1 of t+1
        if constexpr (decltype(VM1)::value == 6) FPM_VMCNT(6);
        else if constexpr (decltype(VM1)::value == 4) FPM_VMCNT(4);
        else if constexpr (decltype(VM1)::value == 2) FPM_VMCNT(2);
        else if constexpr (decltype(VM1)::value == 0) FPM_VMCNT(0);
        if (iss1) issue(phi + 7, SLOT[(1 + 6) & 3]);
        read_b(t, 1, b1);
        mfma(acc[0][1], b1);
        // q2: quadrant (1,1), reads A1; issues A0 of t+2
        if constexpr (decltype(VM2)::value == 6) FPM_VMCNT(6);
        else if constexpr (decltype(VM2)::value == 4) FPM_VMCNT(4);
        else if constexpr (decltype(VM2)::value == 2) FPM_VMCNT(2);
        else if constexpr (decltype(VM2)::value == 0) FPM_VMCNT(0);
        if (iss2) issue(phi + 8, SLOT[(2 + 6) & 3]);
        read_a(t, 1);
        mfma(acc[1][1], b1);
        // q3: quadrant (1,0), no reads; issues B0 of t+2
        if constexpr (decltype(VM3)::value == 6) FPM_VMCNT(6);
        else if constexpr (decltype(VM3)::value == 4) FPM_VMCNT(4);
        else if constexpr (decltype(VM3)::value == 2) FPM_VMCNT(2);
        else if constexpr (decltype(VM3)::value == 0) FPM_VMCNT(0);
        if (iss3) issue(phi + 9, SLOT[(3 + 6) & 3]);
        mfma(acc[1][0], b0);
    };
    using V6 = std::integral_constant<int, 6>;
    using V4 = std::integral_constant<int, 4>;
    using V2 = std::integral_constant<int, 2>;
    using V0 = std::integral_constant<int, 0>;
    using VN = std::integral_constant<int, -1>;

    GP_STAMP(0);
    const int ktiles = p.K / G2_BK;                       // >= GP_MIN_KTILES (checked by the launcher)
    // prologue: half-tiles j = 0..5 (all of K-tile 0, A0 B0 of K-tile 1); A0(0) B0(0) readable first
#pragma unroll
    for (int j = 0; j < 6; ++j) issue(j, SLOT[j & 3]);
    FPM_VMCNT(8);
    __builtin_amdgcn_s_barrier();
    GP_STAMP(1);
    if (GP_STAGGER && wr == 1) __builtin_amdgcn_s_barrier();   // group 1 runs one barrier behind

    // steady state: phase phi retires j = phi + 2 (vmcnt 6) and issues j = phi + 6
    int t = 0;
    for (; t < ktiles - 2; ++t) ktile(t, V6{}, V6{}, V6{}, V6{}, true, true, true, true);
    // K-tile ktiles-2: issues the last two half-tiles (B1, A1 of the last K-tile)
    ktile(t, V6{}, V6{}, V6{}, V4{}, true, true, false, false);
    // last K-tile: retire j = J-2 (vmcnt 2), J-1 (vmcnt 0), then nothing in flight
    ktile(t + 1, V2{}, V0{}, VN{}, VN{}, false, false, false, false);
    if (GP_STAGGER && wr == 0) __builtin_amdgcn_s_barrier();   // re-align the groups
    __syncthreads();
    GP_STAMP(2);

    // epilogue through LDS (same images as gemm_big_kernel<256>)
    int n1b = 0, n2b = 0;
    if (EPI == EPI_AFFINITY) { n1b = p.n1[batch]; n2b = p.n2[batch]; }
    if constexpr (DIRECT) {
        static_assert(!F32OUT && EPI == EPI_STORE, "DIRECT: bf16 output, plain store");
        // lane: output row  h*128 + wr*64 + fm*16 + (lane & 15), columns g*128 + wc*32 + fn*16 + 4*(lane >> 4) + [0, 4)
        bf16_t* Ct = (bf16_t*)p.Ct + (long)batch * p.sC;
        const int cl = wc * 32 + 4 * (lane >> 4);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int fm = 0; fm < 4; ++fm) {
                const int r = row0 + h * 128 + wr * 64 + fm * 16 + (lane & 15);
                if (r >= row_end) continue;
                bf16_t* rowp = Ct + (long)r * p.ldc + n0;
#pragma unroll
                for (int g = 0; g < 2; ++g)
#pragma unroll
                    for (int fn = 0; fn < 2; ++fn) {
                        const int c = g * 128 + cl + fn * 16;
                        if (n0 + c >= p.N) continue;
                        const f32x4_t v = acc[h][g][fm][fn];
                        uint2 o;
                        o.x = f2bf2(v[0], v[1]);
                        o.y = f2bf2(v[2], v[3]);
                        *(uint2*)(rowp + c) = o;
                    }
            }
        return;
    }
    if (!F32OUT) {
        constexpr int ROW = BN * 2 + 16;
        // the bias test hoisted out of the image loop (a compile-time branch each; g2_epi)
        // per-lane base of the image (one per 128-row half, so each write's remaining offset is a
        // compile-time constant within the 16-bit LDS offset field)
        const int lr = wr * 64 + (lane >> 4) * 4, lc = wc * 32 + (lane & 15);
        auto image = [&](auto hb) __attribute__((always_inline)) {
            constexpr bool HB = decltype(hb)::value;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                int wo = (h * 128 + lr) * ROW + lc * 2;
                asm volatile("" : "+v"(wo));        // a base of its own (not h = 0's + a 17-bit constant)
                unsigned char* wb = smem + wo;
#pragma unroll
                for (int g = 0; g < 2; ++g)
#pragma unroll
                    for (int fm = 0; fm < 4; ++fm)
#pragma unroll
                        for (int j = 0; j < 4; j += 2) {     // rows j, j+1: one v_cvt_pk_bf16_f32
                            const int r = h * 128 + lr + fm * 16 + j;
#pragma unroll
                            for (int fn = 0; fn < 2; ++fn) {
                                const int c = g * 128 + lc + fn * 16;
                                const int n = n0 + c < p.N ? n0 + c : p.N - 1;
                                const uint32_t pk =
                                    f2bf2(g2_epi<EPI, HB>(p.bias, acc[h][g][fm][fn][j], row0 + r, n, n1b, n2b),
                                          g2_epi<EPI, HB>(p.bias, acc[h][g][fm][fn][j + 1], row0 + r + 1, n, n1b, n2b));
                                const int off = (fm * 16 + j) * ROW + (g * 128 + fn * 16) * 2;
                                *(bf16_t*)(wb + off) = (bf16_t)pk;
                                *(bf16_t*)(wb + off + ROW) = (bf16_t)(pk >> 16);
                            }
                        }
            }
        };
        if (p.bias) image(std::true_type{});
        else image(std::false_type{});
        __syncthreads();
        GP_STAMP(3);
        bf16_t* Ct = (bf16_t*)p.Ct + (long)batch * p.sC;
        constexpr int CH = BN / 8;
        if (p.store_sc1) {
            // the tile's rows as one buffer resource (256 rows x ldc bf16 < 2 GiB), sc1 stores
            typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
            const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
                (void*)(Ct + (long)row0 * p.ldc + n0), (short)0, (int)(G2_BM * p.ldc * 2), 0x00020000);
#pragma unroll 4
            for (int it = 0; it < G2_BM * CH / G2_THREADS; ++it) {
                const int idx = it * G2_THREADS + tid;
                const int r = idx / CH, ch = idx % CH;
                if (row0 + r < row_end && n0 + ch * 8 < p.N) {
                    const uint4 v = *(const uint4*)(smem + r * ROW + ch * 16);
                    const u32x4_t pk = {v.x, v.y, v.z, v.w};
                    __builtin_amdgcn_raw_buffer_store_b128(pk, rc, (int)((r * p.ldc + ch * 8) * 2), 0, 16);
                }
            }
        } else {
#pragma unroll 4
            for (int it = 0; it < G2_BM * CH / G2_THREADS; ++it) {
                const int idx = it * G2_THREADS + tid;
                const int r = idx / CH, ch = idx % CH;
                if (row0 + r < row_end && n0 + ch * 8 < p.N) {
                    uint4 v = *(const uint4*)(smem + r * ROW + ch * 16);
                    *(uint4*)(Ct + (long)(row0 + r) * p.ldc + n0 + ch * 8) = v;
                }
            }
        }
        GP_STAMP(4);
#ifdef GP_PROBE
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the probe's last stamp: stores retired
        GP_STAMP(5);
#endif
    } else {
        constexpr int ROW = BN * 4 + 16;
        float* Cf = p.Cf + (long)batch * p.sC;
        constexpr int CH = BN / 4;
        auto image = [&](int h, auto hb) __attribute__((always_inline)) {
            constexpr bool HB = decltype(hb)::value;
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int fm = 0; fm < 4; ++fm)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = wr * 64 + fm * 16 + (lane >> 4) * 4 + j;     // row within half h
#pragma unroll
                        for (int fn = 0; fn < 2; ++fn) {
                            const int c = g * 128 + wc * 32 + fn * 16 + (lane & 15);
                            const int n = n0 + c < p.N ? n0 + c : p.N - 1;
                            *(float*)(smem + r * ROW + c * 4) =
                                g2_epi<EPI, HB>(p.bias, acc[h][g][fm][fn][j], row0 + h * 128 + r, n, n1b, n2b);
                        }
                    }
        };
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (p.bias) image(h, std::true_type{});
            else image(h, std::false_type{});
            __syncthreads();
#pragma unroll 4
            for (int it = 0; it < 128 * CH / G2_THREADS; ++it) {
                const int idx = it * G2_THREADS + tid;
                const int r = idx / CH, ch = idx % CH;
                const int gr = row0 + h * 128 + r;
                if (gr < row_end && n0 + ch * 4 < p.N) {
                    uint4 v = *(const uint4*)(smem + r * ROW + ch * 16);
                    *(uint4*)(Cf + (long)gr * p.ldc + n0 + ch * 4) = v;
                }
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Strip walk: the same tile (bf16 output, plain store + optional bias, N % 256 == 0), but a workgroup
// computes S = 1 or 2 consecutive row tiles of one column tile and the LDS-DMA stream runs on across
// the tile boundary, so a tile's prologue (tile table -> a_rows -> first DMA -> first data) and most
// of its epilogue leave the matrix pipe's critical path.  Per element the K order of the MFMA
// accumulation is the phase kernel's, so the outputs stay bit-identical to gemm_big_kernel<256>.
//
// * Grid: ceil(mtiles / S) strips x nt column tiles; strip s runs on XCD s % 8, its nt workgroups
//   next to each other there, so they start together and gather the same A rows (the order of
//   remap_tile with one strip per XCD chunk; larger chunks leave some XCD a round more than the
//   others once a launch is only a few rounds of strips).  The strip's table entries (group, row0,
//   row_end of each step) are read once at the start, so a strip may cross cell groups; a padded
//   tile_info entry (group < 0) is skipped, not the strip's end.
// * K-tile counter u runs over the whole strip; K-tile u lives in buffer u & 1, so the parity is
//   right for any number of K-tiles per tile.  With T K-tiles per tile, the phases of a tile that has
//   a successor issue, in the steady-state order and with the steady-state vmcnt(6):
//       K-tile T-2: q0 B1(T-1)  q1 A1(T-1)  q2 A0(next, 0)  q3 B0(next, 0)
//       K-tile T-1: q0 B1(next, 0)  q1 A1(next, 0)  q2 -  q3 -
//   i.e. the next tile's first K-tile goes where K-tile T-2 was read, by the rule of the steady
//   state (re-staged two phases after the last read).  Its second K-tile would land in the buffer of
//   K-tile T-1, which the epilogue uses, so it waits for the epilogue.  The last tile of a strip
//   drains as the phase kernel does (vmcnt 6 6 6 4 / 2 0 - -).
// * Epilogue inside the buffer of K-tile T-1 (64 KB) while the other buffer holds (or receives) the
//   next tile's first K-tile.  The MFMAs run with swapped operands (weights first), so a lane holds
//   4 consecutive output columns of one row and writes a fragment with one 8-byte LDS write (32 per
//   wave and tile).  The image is written in two 128-row halves of 512 B rows, the 16-byte chunk
//   index XORed with (row & 7): the 16 rows of a write fall on 8 chunk columns (2-way, within the
//   write's own cycles), the 16-byte read-back is conflict-free; each half is stored with whole-row
//   16-byte stores before the next is written.  Barriers (all raw s_barrier, the groups re-aligned):
//       [last MFMA phase] B  write half 0  lgkm0 B  read half 0, store  lgkm0 B  write half 1
//       lgkm0 B  read half 1, store  lgkm0 B  -> the buffer is free
//   WAR: image writes follow a barrier after every wave's last fragment read (lgkmcnt(0) in phase
//   q2 of K-tile T-1); half 1's writes and the DMA re-staging follow a barrier after every wave's
//   lgkmcnt(0) on its image reads.
// * Tile boundary: A0(1) B0(1) of the next tile issued into the freed buffer, then ONE drain per
//   tile, s_waitcnt vmcnt(4): in-order retirement leaves only those four DMA instructions in
//   flight, so the next tile's whole first K-tile (issued two K-tiles earlier) and this tile's
//   global stores have retired -- the stores are counted in vmcnt with the DMA, and this is the
//   one place that accounts for them.  Then a barrier, the stagger barrier of group 1, and the next
//   tile starts in exactly the state the phase kernel's prologue leaves (six half-tiles issued, the
//   first K-tile readable).  The drain costs the store-retire time but never waits for a DMA that
//   was issued less than a K-tile ago.
// * Lookups off the critical path: the strip's table entries come from scalar loads before the first
//   store, and both tiles' a_rows are loaded in the strip's prologue, before any DMA is in flight
//   (a tracked load consumed while LDS-DMA is in flight makes the compiler wait vmcnt(0)).  The
//   compiler also waits vmcnt(0) before the image's first LDS write (it may alias the DMA); by then
//   the youngest DMA is two phases old.
// * Addressing: a uniform base carries the K offset (and B's group and half); the lane adds a
//   32-bit byte offset for B (the same for every tile of the strip; N * ldb * 2 < 2 GiB checked by
//   the launcher) and row * lda + chunk for the gathered A rows, kept as 4 row indices per tile
//   (the row table's range is not known to the launcher, so the sum is formed in 64 bits at issue).
// * Resources (-Rpass-analysis=kernel-resource-usage): 254 VGPRs (256 with sc1 stores), no scratch,
//   131 072 B LDS: two waves per SIMD, as the phase kernel (227 VGPRs, 135 168 B).  The peeled
//   K-tiles take their wait counts and issue modes at run time: a second copy of their MFMAs on the
//   has-successor path made the accumulators meet at a join and spill.
constexpr int GW_SMEM = 8 * GP_HALF;
constexpr int GW_MAX_S = 2;

// Strips are one or two tiles long.  Alone, strips of 3 or 4 were the fastest form of most launches
// (-5 % at 1 270 tiles, -10 % at 640; profiles/r07_gemm_walk.txt section A), but inside the
// forward's two-stream pipeline they gave nothing back (the GPU stage within +-0.4 % of one tile per
// workgroup, section B) where strips of 2 kept their gain: the other stream's kernels cannot enter
// a CU before a strip ends.  So the kernel carries no state for a third tile.
// Strips of 2 are taken when their rounds cost less than the single tiles' rounds: a tile inside a
// strip takes 7/8 of a workgroup of the phase kernel (41.6 K against 48.4 K clocks, "probe" rows of
// section F), but pairing rounds the launch up to whole strips -- 2 ceil(strips wgs / CUs) tile
// times against ceil(tiles wgs / CUs).  335 tiles x 3 column tiles: 4 against 4 rounds, -17 %;
// 180 x 3: 4 against 3, +12 % if forced; 65 x 1: 2 against 1, +60 % if forced (same file).  The
// kernel decides, with the real tile count of a grouped launch (the host knows only the table's
// worst-case size).
__host__ __device__ inline int gemm_walk_rule(int tiles, int wgs, int cus) {
    const long r1 = ((long)tiles * wgs + cus - 1) / cus, r2 = ((long)((tiles + 1) / 2) * wgs + cus - 1) / cus;
    return 2 * r2 * 7 <= r1 * 8 ? 2 : 1;
}

#ifdef GP_PROBE
// walk stamps, first tile of a strip of two: 0 main loop start, 1 next tile's first DMA issued, 2
// main loop end, 3 image written and stores issued (buffer free), 4 next tile's first K-tile landed
#define GW_STAMP(k) do { if (ti == 0) GP_STAMP(k); } while (0)
#else
#define GW_STAMP(k)
#endif

template <bool SC1>
__global__ __launch_bounds__(G2_THREADS, 1) void gemm_walk_kernel(GemmParams p) {
    constexpr int BN = 256;
    __shared__ __attribute__((aligned(16))) unsigned char smem[GW_SMEM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 2, wc = wave & 3;
    const int batch = blockIdx.z;

    const int nt = p.N / BN;
    // real row tiles of the launch: a grouped launch's table is sized for the worst case, the plan
    // leaves the count it filled next to it
    int mtiles = p.remap_mtiles;
    if (p.tile_count) mtiles = *p.tile_count < mtiles ? *p.tile_count : mtiles;
    const int S = p.walk > 0 ? p.walk : gemm_walk_rule(mtiles, nt * (int)gridDim.z, p.walk_cus);
    const int strips = (mtiles + S - 1) / S;
    // strip s runs on XCD s % 8 (workgroups go to the XCDs round-robin by blockIdx), its nt
    // workgroups next to each other there: they start together and gather the same A rows.
    // The grid is sized for S = 1 unless the host forced strips of 2; the surplus exits here
    const int i = blockIdx.x >> 3;
    const int strip = (i / nt) * 8 + (blockIdx.x & 7), ntile = i % nt;
    if (strip >= strips) return;
    // The strip's table entries are read once, here, before the kernel's first store: scalar loads
    // (after a store the compiler reads the table with vector loads and waits vmcnt(0) for each,
    // which would put two dependent memory round trips, and a drain, on every tile boundary).
    // Bit j of ok: step j of the strip is a real tile (padded entries are skipped, not the end).
    int t_row0[GW_MAX_S], t_rend[GW_MAX_S], t_grp[GW_MAX_S];
    unsigned ok = 0;
#pragma unroll
    for (int j = 0; j < GW_MAX_S; ++j) {
        const int mt = strip * S + j;
        t_row0[j] = 0; t_rend[j] = 0; t_grp[j] = 0;
        if (j < S && mt < mtiles) {
            if (p.tile_info) {
                const int g = p.tile_info[2 * mt];
                if (g >= 0) {
                    t_grp[j] = g;
                    t_row0[j] = p.tile_info[2 * mt + 1];
                    t_rend[j] = p.group_off[g + 1];
                    ok |= 1u << j;
                }
            } else {
                t_row0[j] = mt * G2_BM;
                t_rend[j] = p.M;
                ok |= 1u << j;
            }
        }
    }
    if (!ok) return;
    constexpr int m_end = GW_MAX_S;
    // first real step at or after j
    auto next_valid = [&](int j) __attribute__((always_inline)) {
        const unsigned r = j < GW_MAX_S ? ok >> j : 0u;
        return r ? j + __builtin_ctz(r) : GW_MAX_S;
    };
    auto pick = [&](const int (&t)[GW_MAX_S], int j) __attribute__((always_inline)) {
        return j == 0 ? t[0] : t[1];
    };
    int m = next_valid(0);

    const int n0 = ntile * BN;
    const bf16_t* A = (const bf16_t*)p.A + (long)batch * p.sA;
    const unsigned char* Bb = (const unsigned char*)((const bf16_t*)p.B + (long)batch * p.sB);
    bf16_t* Ct = (bf16_t*)p.Ct + (long)batch * p.sC;

    // per step (all wave-uniform): rows [row0, row_end), B of the tile's group
    auto tile_at = [&](int j, int& row0, int& row_end, const unsigned char*& bg) __attribute__((always_inline)) {
        row0 = pick(t_row0, j);
        row_end = pick(t_rend, j);
        bg = Bb + (long)pick(t_grp, j) * p.sB_seg * 2;
    };
    // DMA sources: half-tile piece i of wave w = rows 8*(2w+i) + (lane>>3) of the half,
    // K-chunk (lane&7) ^ ((row>>1)&7)
    auto a_rows_of = [&](int row0, int row_end, int (&ar)[2][2]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                int gr = row0 + h * 128 + (wave * 2 + i) * 8 + (lane >> 3);
                gr = gr < row_end ? gr : row0;            // clamp: rows past the end are never stored
                ar[h][i] = p.a_rows ? p.a_rows[gr] : gr;
            }
    };
    // byte offset of the lane's 16-byte K-chunk in its row: piece 1 sits 8 rows below piece 0, its
    // chunk is piece 0's ^ 4
    const uint32_t kc16 = (uint32_t)(((lane & 7) ^ (lane >> 4)) * 16);
    uint32_t b_off[2];                                    // [piece], bytes from the B of half 0
#pragma unroll
    for (int i = 0; i < 2; ++i)
        b_off[i] = (uint32_t)((n0 + (wave * 2 + i) * 8 + (lane >> 3)) * (uint32_t)p.ldb * 2) + (kc16 ^ (i * 64));
    const uint32_t lda2 = (uint32_t)p.lda * 2, bhalf = 128 * (uint32_t)p.ldb * 2;
    const unsigned char* Ab = (const unsigned char*)A;

    int row0, row_end, row0n = 0, row_endn = 0;
    const unsigned char *bg, *bgn = nullptr;
    int ar[2][2], arn[2][2];                              // gathered A rows [half][piece]: tile, next tile

    // one half-tile (slot 0 1 2 3 = A0 A1 B0 B1) of the K-tile at element offset k0 into buffer buf:
    // a uniform base that carries the K offset (and B's group and half) plus the lane's offset --
    // 32 bits for B, row * lda + chunk in 64 bits for the gathered A rows
    auto issue = [&](int slot, int buf, const int (&rows)[2][2], const unsigned char* bgrp, int k0) __attribute__((always_inline)) {
        unsigned char* dst = smem + (buf * 4 + slot) * GP_HALF + wave * 2048;
        if (slot < 2) {
            const unsigned char* ab = Ab + 2 * k0;
#pragma unroll
            for (int i = 0; i < 2; ++i)
                __builtin_amdgcn_global_load_lds(
                    (gbl_ptr_t)(ab + ((uint64_t)(uint32_t)rows[slot][i] * lda2 + (kc16 ^ (i * 64)))),
                    (lds_ptr_t)(dst + i * 1024), 16, 0, 0);
        } else {
            const unsigned char* b = bgrp + 2 * k0 + (slot - 2) * bhalf;
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(b + b_off[0]), (lds_ptr_t)dst, 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(b + b_off[1]), (lds_ptr_t)(dst + 1024), 16, 0, 0);
        }
    };

    // fragment reads as in gemm_phase_kernel
    const int xr = (lane >> 1) & 7;
    const int a_off = (wr * 64 + (lane & 15)) * 128;
    const int b_offl = (wc * 32 + (lane & 15)) * 128;
    const int s0 = ((lane >> 4) ^ xr) * 16, s1 = ((4 + (lane >> 4)) ^ xr) * 16;

    f32x4_t acc[2][2][4][2];                              // [h][g][fm][fn]
    auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[h][g][i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    };
    bf16x8_t a[2][4], b0[2][2], b1[2][2];                 // [kk][frag]

    auto read_a = [&](int u, int h) __attribute__((always_inline)) {
        const unsigned char* base = smem + ((u & 1) * 4 + h) * GP_HALF + a_off;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            a[0][f] = *(const bf16x8_t*)(base + f * 2048 + s0);
            a[1][f] = *(const bf16x8_t*)(base + f * 2048 + s1);
        }
    };
    auto read_b = [&](int u, int g, bf16x8_t (&bb)[2][2]) __attribute__((always_inline)) {
        const unsigned char* base = smem + ((u & 1) * 4 + 2 + g) * GP_HALF + b_offl;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            bb[0][f] = *(const bf16x8_t*)(base + f * 2048 + s0);
            bb[1][f] = *(const bf16x8_t*)(base + f * 2048 + s1);
        }
    };
    // swapped operands: the lane's accumulator holds output row (lane & 15), columns 4*(lane>>4)+[0,4)
    auto mfma = [&](f32x4_t (&c)[4][2], bf16x8_t (&bb)[2][2]) __attribute__((always_inline)) {
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (GP_PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int fm = 0; fm < 4; ++fm)
#pragma unroll
                for (int fn = 0; fn < 2; ++fn)
                    c[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bb[kk][fn], a[kk][fm], c[fm][fn], 0, 0, 0);
        if (GP_PRIO) __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_s_barrier();
    };
    // modes of a phase pair's issues: nothing, this tile's K-tile at k0, the next tile's first K-tile
    constexpr int NONE = 0, CUR = 1, NEXT = 2;
    // the peeled K-tiles pick count and mode by has_next at run time (scalar branches round the wait
    // and the issue only: one copy of each K-tile's MFMAs, the accumulators never meet at a join)
    auto wait = [&](int v) __attribute__((always_inline)) {
        if (v == 6) FPM_VMCNT(6);
        else if (v == 4) FPM_VMCNT(4);
        else if (v == 2) FPM_VMCNT(2);
        else if (v == 0) FPM_VMCNT(0);
    };
    auto iss = [&](int mode, int slot, int buf, int k0) __attribute__((always_inline)) {
        if (mode == CUR) issue(slot, buf, ar, bg, k0);
        else if (mode == NEXT) issue(slot, buf, arn, bgn, 0);
    };
    // K-tile u of the strip (buffer u & 1), k1 = element offset of this tile's next K-tile: phases
    // q0 q1 stage B1 A1 of K-tile u + 1 (mode M01), q2 q3 stage A0 B0 of K-tile u + 2 (mode M23)
    auto ktile = [&](int u, int k1, int VM0, int VM1, int VM2, int VM3, int M01, int M23) __attribute__((always_inline)) {
        asm volatile("" : "+s"(k1));                      // no per-lane pointer induction: bases stay scalar
        wait(VM0);
        iss(M01, 3, (u + 1) & 1, k1);
        read_a(u, 0);
        read_b(u, 0, b0);
        mfma(acc[0][0], b0);                              // q0: quadrant (0,0), reads A0 + B0
        wait(VM1);
        iss(M01, 1, (u + 1) & 1, k1);
        read_b(u, 1, b1);
        mfma(acc[0][1], b1);                              // q1: quadrant (0,1), reads B1
        wait(VM2);
        iss(M23, 0, u & 1, k1 + G2_BK);
        read_a(u, 1);
        mfma(acc[1][1], b1);                              // q2: quadrant (1,1), reads A1
        wait(VM3);
        iss(M23, 2, u & 1, k1 + G2_BK);
        mfma(acc[1][0], b0);                              // q3: quadrant (1,0), no reads
    };

    // image addressing: half-row rr = wr*64 + fm*16 + (lane & 15), 16-byte chunk c at c ^ (rr & 7)
    // (rr & 7 == lane & 7); a lane's 8 bytes are columns g*128 + wc*32 + fn*16 + 4*(lane>>4) + [0,4)
    // read-back: thread -> half-row it*16 + (tid >> 5), chunk tid & 31.  The lane's bases are worked
    // out here, once per tile, from an opaque copy of tid, so they do not hold registers in the K loop
    auto epilogue = [&](int buf, auto hb) __attribute__((always_inline)) {
        constexpr bool HB = decltype(hb)::value;
        unsigned char* img = smem + buf * (4 * GP_HALF);
        int tid_ = tid;
        asm volatile("" : "+v"(tid_));
        const int lane = tid_ & 63, wr = tid_ >> 8, wc = (tid_ >> 6) & 3;
        int wbase[2];
#pragma unroll
        for (int fn = 0; fn < 2; ++fn)
            wbase[fn] = (wr * 64 + (lane & 15)) * 512 + (((wc * 4 + fn * 2 + (lane >> 5)) ^ (lane & 7)) << 4) +
                        ((lane >> 4) & 1) * 8;
        const int rb_r = tid_ >> 5, rb_c = tid_ & 31;
        const int rbase = rb_r * 512 + ((rb_c ^ (rb_r & 7)) << 4);
        const int cl = n0 + wc * 32 + 4 * (lane >> 4);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int fm = 0; fm < 4; ++fm)
#pragma unroll
                    for (int fn = 0; fn < 2; ++fn) {
                        const f32x4_t v = acc[h][g][fm][fn];
                        const int n = cl + g * 128 + fn * 16;
                        uint2 o;
                        o.x = f2bf2(g2_epi<EPI_STORE, HB>(p.bias, v[0], 0, n, 0, 0),
                                    g2_epi<EPI_STORE, HB>(p.bias, v[1], 0, n + 1, 0, 0));
                        o.y = f2bf2(g2_epi<EPI_STORE, HB>(p.bias, v[2], 0, n + 2, 0, 0),
                                    g2_epi<EPI_STORE, HB>(p.bias, v[3], 0, n + 3, 0, 0));
                        *(uint2*)(img + wbase[fn] + fm * 8192 + g * 256) = o;
                    }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const int rbeg = row0 + h * 128 + rb_r;
            if constexpr (SC1) {
                // the tile's rows as one buffer resource (256 rows x ldc bf16 < 2 GiB), sc1 stores
                typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
                const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
                    (void*)(Ct + (long)row0 * p.ldc + n0), (short)0, (int)(G2_BM * p.ldc * 2), 0x00020000);
#pragma unroll
                for (int it = 0; it < 8; ++it) {
                    const uint4 v = *(const uint4*)(img + rbase + it * 8192);
                    if (rbeg + it * 16 < row_end) {
                        const u32x4_t pk = {v.x, v.y, v.z, v.w};
                        __builtin_amdgcn_raw_buffer_store_b128(
                            pk, rc, (int)(((h * 128 + rb_r + it * 16) * p.ldc + rb_c * 8) * 2), 0, 16);
                    }
                }
            } else {
#pragma unroll
                for (int it = 0; it < 8; ++it) {
                    const uint4 v = *(const uint4*)(img + rbase + it * 8192);
                    if (rbeg + it * 16 < row_end) *(uint4*)(Ct + (long)(rbeg + it * 16) * p.ldc + n0 + rb_c * 8) = v;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
    };

    const int T = p.K / G2_BK;                            // >= GP_MIN_KTILES (checked by the launcher)
    // strip prologue: this tile's and the next tile's sources, then half-tiles j = 0..5
    tile_at(m, row0, row_end, bg);
    a_rows_of(row0, row_end, ar);
    int mn = next_valid(m + 1);
    if (mn < m_end) {
        tile_at(mn, row0n, row_endn, bgn);
        a_rows_of(row0n, row_endn, arn);
    }
    issue(0, 0, ar, bg, 0);
    issue(2, 0, ar, bg, 0);
    issue(3, 0, ar, bg, 0);
    issue(1, 0, ar, bg, 0);
    issue(0, 1, ar, bg, G2_BK);
    issue(2, 1, ar, bg, G2_BK);
    zero_acc();
    FPM_VMCNT(8);
    __builtin_amdgcn_s_barrier();

    int u = 0;
#ifdef GP_PROBE
    int ti = 0;
#endif
    for (;;) {
        // here: six half-tiles of this tile issued, its first K-tile's A0 B0 readable, acc zero
        const bool has_next = mn < m_end;
        GW_STAMP(0);
        if (GP_STAGGER && wr == 1) __builtin_amdgcn_s_barrier();   // group 1 runs one barrier behind
        int k1 = G2_BK;
        for (int t = 0; t < T - 2; ++t, ++u, k1 += G2_BK) ktile(u, k1, 6, 6, 6, 6, CUR, CUR);
        // K-tile T-2: the next tile's A0 B0, or the drain's first step (vmcnt 4: nothing issued in q2)
        ktile(u, k1, 6, 6, 6, has_next ? 6 : 4, CUR, has_next ? NEXT : NONE);
        GW_STAMP(1);
        // K-tile T-1: the next tile's B1 A1, or the drain (vmcnt 2, 0)
        ktile(u + 1, 0, has_next ? 6 : 2, has_next ? 6 : 0, -1, -1, has_next ? NEXT : NONE, NONE);
        ++u;                                              // the tile's last K-tile: the image's buffer
        if (GP_STAGGER && wr == 0) __builtin_amdgcn_s_barrier();   // re-align the groups
        GW_STAMP(2);
        if (p.bias) epilogue(u & 1, std::true_type{});
        else epilogue(u & 1, std::false_type{});
        GW_STAMP(3);
        if (!has_next) break;
        // tile boundary: the successor becomes the tile (the strip's last: both tiles' rows were
        // loaded in the prologue, no load is in flight here), A0 B0 of its second K-tile go into
        // the freed buffer, one drain
        m = mn; mn = m_end;
        row0 = row0n; row_end = row_endn; bg = bgn;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 2; ++i) ar[h][i] = arn[h][i];
        issue(0, u & 1, ar, bg, G2_BK);
        issue(2, u & 1, ar, bg, G2_BK);
        FPM_VMCNT(4);
        zero_acc();
        __builtin_amdgcn_s_barrier();
        GW_STAMP(4);
        ++u;
#ifdef GP_PROBE
        ++ti;
#endif
    }
}

#undef FPM_VMCNT

// launch policy: the phase kernel for 256-wide tiles with >= 2 K-tiles; FPM_GEMM_PHASE=0 (or
// fpm_set_gemm_phase(0)) keeps gemm_big_kernel<256> -- an A/B switch, both are bit-identical
int& gemm_phase_flag();
inline bool use_gemm_phase(int K) { return gemm_phase_flag() != 0 && K / G2_BK >= GP_MIN_KTILES; }

// fpm_set_tuning("gemm_walk", v) / FPM_GEMM_WALK: 0, 1 = off (the phase kernel), 2..7 = strips of 2
// forced, default GW_AUTO = gemm_walk_rule, evaluated by the kernel (tuning values are not
// negative: fpm_set_tuning returns the previous one, -1 is its error).  When the rule picks S = 1
// the launch still runs on the walk kernel, as strips of one tile (prologue, tile, drain; the
// swapped-operand epilogue) -- bit-identical, not the phase kernel itself; only 0 and 1 give that.
constexpr int GW_AUTO = 8;
int& gemm_walk_flag();
int gemm_cu_count();
// 0 = the phase kernel takes this launch; else the walk kernel: 2 = strips of 2 forced, GW_AUTO =
// the rule (bf16 EPI_STORE tiles of the phase kernel, N % 256 == 0)
inline int gemm_walk_strip(const GemmParams& p) {
    const int f = gemm_walk_flag();
    if (f <= 1 || !use_gemm_phase(p.K) || p.N % 256 != 0 || !p.Ct || p.Cf || p.epi != EPI_STORE) return 0;
    // 32-bit lane offsets into B and into a tile's output rows, 32-bit lda
    if ((long)p.N * p.ldb * 2 >= (1L << 31) || (long)G2_BM * p.ldc * 2 >= (1L << 31) || p.lda >= (1L << 31)) return 0;
    return f < GW_AUTO ? 2 : GW_AUTO;
}
inline void gemm_walk_launch(GemmParams p, int S, int batch, hipStream_t st) {
    const long nt = p.N / 256;
    p.walk_cus = gemm_cu_count();
    // Under the rule, a launch of eight rounds or more by its table's size (for a grouped launch the
    // worst case, about 2.5 times the real count; from three real rounds on the rounding costs
    // strips of 2 less than they gain) is given strips of 2 here: the grid is sized for them, which
    // halves the workgroups that only find the table's padding and exit (2.4 ns each, a few
    // thousand per launch).  A smaller launch is left to the kernel (p.walk = 0, grid for S = 1)
    p.walk = S == 2 || p.remap_mtiles * nt * batch >= 8L * gemm_cu_count() ? 2 : 0;
    const int strips = p.walk ? (p.remap_mtiles + 1) / 2 : p.remap_mtiles;
    const dim3 grid((unsigned)((strips + 7) / 8 * 8 * nt), 1, batch);
    if (p.store_sc1) hipLaunchKernelGGL((gemm_walk_kernel<true>), grid, dim3(G2_THREADS), 0, st, p);
    else hipLaunchKernelGGL((gemm_walk_kernel<false>), grid, dim3(G2_THREADS), 0, st, p);
}

}  // namespace fpm

// SplineConv message passing (PyG 1.6.3 SplineConv(768, 768, dim=2, kernel_size=5, aggr='max')
// as used by the reference's SConv, src/model/spline_conv.py:17,28-41, and the Siamese
// residual x + 0.1*SConv(x), spline_conv.py:51-57).
//
// MI355X design.  A message is msg_e = sum_s basis[e,s] * (x_src W_{cell(e,s)}) over the 4 corners
// of the edge's B-spline group.  The products x_u W_k depend only on (source node, cell), and the
// ~6 out-edges x 4 corners of a node touch only ~9 distinct cells (neighbouring directions share
// cells), so each needed (node, cell) product is computed ONCE: the plan marks a 26-bit cell mask
// per node (25 spline cells + the root weight as cell 25), ranks the (node, cell) rows per cell in
// node order, and one grouped MFMA GEMM (group = cell, A = gathered node rows, B = that cell's
// [out][in] weight; bf16: the 256x256 LDS-DMA tile of gemm_big.h) writes the product rows Y.  A combine kernel then forms each in-edge's message
// from 4 rows of Y in fp32 (basis order s = 0..3, the reference's), takes the max per destination
// and fuses root + bias + ReLU or the Siamese residual.  That is ~2.5x fewer MFMA flops than the
// per-edge GEMM, and the message tensor is never materialised.  The plan (dst CSR included) is
// built on device once per side and shared by both layers and the GNN layers.
#include "gemm_phase.h"

#include <vector>

namespace {

// optional HIP-event timing of the dominant kernel (the (node, cell) product GEMM), read by bench.py
struct ProfRec {
    hipEvent_t a, b;
    int slot;                // g_prof_rows[slot] = product rows of the launch (flops = 2 rows 768^2)
};
bool g_prof_on = false;
std::vector<ProfRec> g_prof;
int* g_prof_rows = nullptr;   // device copies of each profiled launch's row count
constexpr int PROF_MAX = 4096;

constexpr int NCELL = 26;   // 25 B-spline cells + the root weight (cell 25)

struct PlanLayout {
    long mask, indeg, dslot, basis_e, grp_e, blk_cnt, cell_off, rowid, arows, tile_info, tile_info2, dst_ptr, csr_e,
        nbr_local, rows4, basis4, total;
    long nblk, max_rows, max_tiles, max_tiles2;
};

__host__ __device__ inline long al(long x) { return (x + 255) & ~255L; }

// Deduplicated message GEMM: every (source node, cell) product x_u W_k that some edge corner needs
// is computed once (a node's ~6 out-edges x 4 corners touch ~9 distinct cells), root = cell 25.
__host__ __device__ inline long plan_max_rows(long E, long num_nodes) {
    long a = 4 * E, b = 25 * num_nodes;
    return (a < b ? a : b) + num_nodes;
}

__host__ __device__ PlanLayout plan_layout(long E, long num_nodes) {
    PlanLayout L;
    L.nblk = (num_nodes + 255) / 256;
    L.max_rows = plan_max_rows(E, num_nodes);
    L.max_tiles = L.max_rows / fpm::GBM + NCELL + 1;      // 128-row tiles (fp32 kernel)
    L.max_tiles2 = L.max_rows / fpm::G2_BM + NCELL + 1;   // 256-row tiles (bf16 kernel)
    long o = 0;
    L.mask = o; o += al(num_nodes * 4);
    L.indeg = o; o += al(num_nodes * 4);
    L.dslot = o; o += al(E * 4);
    L.basis_e = o; o += al(E * 16);
    L.grp_e = o; o += al(E * 4);
    L.blk_cnt = o; o += al(L.nblk * NCELL * 4);
    L.cell_off = o; o += al(32 * 4);
    L.rowid = o; o += al(num_nodes * NCELL * 4);
    L.arows = o; o += al(L.max_rows * 4);
    L.tile_info = o; o += al(L.max_tiles * 8);
    L.tile_info2 = o; o += al(L.max_tiles2 * 8);
    L.dst_ptr = o; o += al((num_nodes + 1) * 4);
    L.csr_e = o; o += al(E * 4);
    L.nbr_local = o; o += al(E * 4);
    L.rows4 = o; o += al(E * 16);
    L.basis4 = o; o += al(E * 16);
    L.total = o;
    return L;
}

// per edge: torch-spline-conv open-spline degree-1 basis, group, the source's cell mask, in-degree slot
__global__ __launch_bounds__(256) void plan_edge_kernel(const int* __restrict__ src, const int* __restrict__ dst,
                                                        const float* __restrict__ pseudo, long E, int* mask,
                                                        int* indeg, int* dslot, float* basis_e, int* grp_e) {
    const long e0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = e0 < E;
    const long e = live ? e0 : E - 1;
    int f[2];
    float fr[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        float v = pseudo[2 * e + d] * 4.0f;
        float fl = floorf(v);
        f[d] = (int)fl;
        fr[d] = v - fl;
    }
    float b4[4];
    int bits = 0;
    const int g = f[0] + 5 * f[1];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float b = 1.0f;
        b = b * ((s & 1) ? fr[0] : 1.0f - fr[0]);
        b = b * ((s >> 1) ? fr[1] : 1.0f - fr[1]);
        b4[s] = b;
        bits |= 1 << fpm::spline_cell(g, s);
    }
    // the source's cell mask: OR the bits of the lanes that share the source (edge lists are
    // grouped by source, so runs are contiguous) into the run's first lane, one atomic per run
    const int key = live ? src[e] : -1;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int kb = __shfl_down(key, o), bb = __shfl_down(bits, o);
        if (lane + o < 64 && kb == key) bits |= bb;
    }
    const int kprev = __shfl_up(key, 1);
    if (!live) return;
    grp_e[e] = g;
    *(float4*)(basis_e + 4 * e) = make_float4(b4[0], b4[1], b4[2], b4[3]);
    if (lane == 0 || kprev != key) atomicOr(&mask[key], bits);
    dslot[e] = atomicAdd(&indeg[dst[e]], 1);
}

// rows of cell k are the nodes whose mask has bit k, in node order (deterministic): per-block
// counts here, block bases by the scan kernel, ranks by plan_rank_kernel (same ballots).
__device__ __forceinline__ unsigned long long cell_ballot(int m, int k) {
    return __ballot((m >> k) & 1);
}

__global__ __launch_bounds__(256) void plan_blkcount_kernel(const int* __restrict__ mask, long num_nodes,
                                                            int* __restrict__ blk_cnt) {
    __shared__ int wc[4][NCELL];
    const long u = (long)blockIdx.x * 256 + threadIdx.x;
    const int m = u < num_nodes ? (mask[u] | (1 << 25)) : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < NCELL; ++k) {
        unsigned long long b = cell_ballot(m, k);
        if (lane == 0) wc[wave][k] = __popcll(b);
    }
    __syncthreads();
    if (threadIdx.x < NCELL) {
        int k = threadIdx.x;
        blk_cnt[(long)blockIdx.x * NCELL + k] = wc[0][k] + wc[1][k] + wc[2][k] + wc[3][k];
    }
}

// one block: per-cell exclusive scan over blocks (in place), cell offsets, GEMM tile table, and the
// exclusive scan of in-degrees -> dst CSR pointers.
// The number of real tiles is also stored at *count (cell_off[27] for 128-row tiles, [28] for
// 256-row tiles).
__device__ void build_tile_table(const int* coff, const int* cell_tot, int* tile_off, int tb, int* tile_info,
                                 int max_tiles, int* count) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        int t = 0;
        for (int k = 0; k < NCELL; ++k) {
            tile_off[k] = t;
            t += (cell_tot[k] + tb - 1) / tb;
        }
        tile_off[NCELL] = t;
        *count = t;
    }
    __syncthreads();
    for (int t = tid; t < max_tiles; t += blockDim.x) {
        int g = -1, r0 = 0;
        if (t < tile_off[NCELL]) {
            int k = 0;
            while (tile_off[k + 1] <= t) ++k;
            g = k;
            r0 = coff[k] + (t - tile_off[k]) * tb;
        }
        tile_info[2 * t] = g;
        tile_info[2 * t + 1] = r0;
    }
    __syncthreads();
}

__global__ __launch_bounds__(1024) void plan_scan_kernel(int* blk_cnt, long nblk, int* cell_off, int* tile_info,
                                                         int max_tiles, int* tile_info2, int max_tiles2,
                                                         const int* indeg, int* dst_ptr, long num_nodes) {
    __shared__ int part[1024];
    __shared__ int tilebuf[16384];
    __shared__ int cell_tot[NCELL], tile_off[NCELL + 1], coff[NCELL + 1];
    const int tid = threadIdx.x;
    // (1) per-cell exclusive scans over blocks: one wave per cell, 64 entries per step via shuffles
    //     (no block-wide barriers on this serial path)
    {
        const int lane = tid & 63, wv = tid >> 6;
        for (int k = wv; k < NCELL; k += 16) {
            int carry = 0;
            for (long t0 = 0; t0 < nblk; t0 += 64) {
                const long i = t0 + lane;
                const int v = i < nblk ? blk_cnt[i * NCELL + k] : 0;
                int incl = v;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int y = __shfl_up(incl, o);
                    if (lane >= o) incl += y;
                }
                if (i < nblk) blk_cnt[i * NCELL + k] = carry + incl - v;
                carry += __shfl(incl, 63);
            }
            if (lane == 0) cell_tot[k] = carry;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int off = 0;
        for (int k = 0; k < NCELL; ++k) {
            cell_off[k] = off;
            coff[k] = off;
            off += cell_tot[k];
        }
        cell_off[NCELL] = off;
        coff[NCELL] = off;
    }
    __syncthreads();
    build_tile_table(coff, cell_tot, tile_off, fpm::GBM, tile_info, max_tiles, cell_off + NCELL + 1);
    build_tile_table(coff, cell_tot, tile_off, fpm::G2_BM, tile_info2, max_tiles2, cell_off + NCELL + 2);
    // (2) exclusive scan of indeg -> dst_ptr, tiled through LDS (coalesced global reads/writes)
    constexpr int TILE = 16384, PER = TILE / 1024;
    int* buf = tilebuf;
    int carry = 0;
    for (long t0 = 0; t0 < num_nodes; t0 += TILE) {
        const int len = (int)(num_nodes - t0 < TILE ? num_nodes - t0 : TILE);
        for (int k = tid; k < TILE; k += 1024) buf[k] = k < len ? indeg[t0 + k] : 0;
        __syncthreads();
        int loc[PER];
        int s = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            loc[k] = s;
            s += buf[tid * PER + k];
        }
        part[tid] = s;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            int v = tid >= o ? part[tid - o] : 0;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        const int base = carry + part[tid] - s;
#pragma unroll
        for (int k = 0; k < PER; ++k) buf[tid * PER + k] = base + loc[k];
        const int total = part[1023];
        __syncthreads();
        for (int k = tid; k < len; k += 1024) dst_ptr[t0 + k] = buf[k];
        carry += total;
        __syncthreads();
    }
    if (tid == 0) dst_ptr[num_nodes] = carry;
}

// rowid[u][k] (or -1) and the GEMM's row gather arows[row] = u
__global__ __launch_bounds__(256) void plan_rank_kernel(const int* __restrict__ mask, long num_nodes,
                                                        const int* __restrict__ blk_base,
                                                        const int* __restrict__ cell_off, int* __restrict__ rowid,
                                                        int* __restrict__ arows) {
    __shared__ int wc[4][NCELL];
    const long u = (long)blockIdx.x * 256 + threadIdx.x;
    const int m = u < num_nodes ? (mask[u] | (1 << 25)) : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int myrank[NCELL];
#pragma unroll
    for (int k = 0; k < NCELL; ++k) {
        unsigned long long b = cell_ballot(m, k);
        if (lane == 0) wc[wave][k] = __popcll(b);
        myrank[k] = __popcll(b & lt);
    }
    __syncthreads();
    if (u >= num_nodes) return;
#pragma unroll
    for (int k = 0; k < NCELL; ++k) {
        int r = -1;
        if ((m >> k) & 1) {
            int pre = 0;
            for (int w = 0; w < wave; ++w) pre += wc[w][k];
            r = cell_off[k] + blk_base[(long)blockIdx.x * NCELL + k] + pre + myrank[k];
            arows[r] = (int)u;
        }
        rowid[u * NCELL + k] = r;
    }
}

__global__ void plan_fill_kernel(const int* __restrict__ src, const int* __restrict__ dst, long E, int nmax,
                                 const int* __restrict__ dslot, const int* __restrict__ dst_ptr, int* csr_e,
                                 int* nbr_local) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    int p = dst_ptr[dst[e]] + dslot[e];
    csr_e[p] = (int)e;
    nbr_local[p] = src[e] % nmax;
}

// Deterministic in-edge order per node (ascending source): the atomics above fill each list in
// arbitrary order, and the max / the GNN aggregation read these lists in order.
__global__ void plan_sort_kernel(const int* __restrict__ dst_ptr, long num_nodes, int* __restrict__ csr_e,
                                 int* __restrict__ nbr_local) {
    long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= num_nodes) return;
    const int beg = dst_ptr[v], end = dst_ptr[v + 1];
    for (int a = beg + 1; a < end; ++a) {
        int kn = nbr_local[a], ke = csr_e[a];
        int b = a - 1;
        while (b >= beg && (nbr_local[b] > kn || (nbr_local[b] == kn && csr_e[b] > ke))) {
            nbr_local[b + 1] = nbr_local[b];
            csr_e[b + 1] = csr_e[b];
            --b;
        }
        nbr_local[b + 1] = kn;
        csr_e[b + 1] = ke;
    }
}

// CSR slot -> the 4 product rows (source node x corner cell) and the 4 basis weights
__global__ void plan_expand_kernel(const int* __restrict__ src, const int* __restrict__ csr_e, long E,
                                   const int* __restrict__ grp_e, const float* __restrict__ basis_e,
                                   const int* __restrict__ rowid, int4* __restrict__ rows4,
                                   float4* __restrict__ basis4) {
    long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    const int e = csr_e[p];
    const int g = grp_e[e];
    const long s = src[e];
    int4 r;
    r.x = rowid[s * NCELL + fpm::spline_cell(g, 0)];
    r.y = rowid[s * NCELL + fpm::spline_cell(g, 1)];
    r.z = rowid[s * NCELL + fpm::spline_cell(g, 2)];
    r.w = rowid[s * NCELL + fpm::spline_cell(g, 3)];
    rows4[p] = r;
    basis4[p] = *(const float4*)(basis_e + 4 * (long)e);
}

// ---- per-graph plan (graphs of <= 4096 directed edges and <= 1024 nodes) ---------------------
// The same plan as the global kernels above, built one workgroup per graph with LDS instead of
// device-wide atomics: a graph's edges are a contiguous range (every batch builder groups them by
// graph, so src is non-decreasing across graph boundaries and the range is found by binary
// search), its nodes are [g nmax, (g + 1) nmax), and its dst CSR occupies exactly its edge range.
// Output fields and orders are identical (cell rows in node order, in-edges by ascending source
// then edge id), so everything downstream is bit-identical to the global path.
constexpr int PG_MAXE = 4096, PG_MAXN = 1024, PG_THREADS = 512;

__device__ __forceinline__ long pg_lower_bound(const int* __restrict__ a, long n, int v) {
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// K1: edge basis / group, node cell masks, per-graph cell counts, dst CSR (sorted in LDS)
__device__ __forceinline__ void plan_graph_body(int g, const int* __restrict__ src, const int* __restrict__ dst,
                                                const float* __restrict__ pseudo, long E, int nmax, int ngraphs,
                                                int* __restrict__ mask, float* __restrict__ basis_e,
                                                int* __restrict__ grp_e, int* __restrict__ cellcnt,
                                                int* __restrict__ dst_ptr, int* __restrict__ csr_e,
                                                int* __restrict__ nbr_local, int* __restrict__ eoff) {
    __shared__ unsigned key[PG_MAXE];
    __shared__ int maskL[PG_MAXN], cnt[PG_MAXN], pos[PG_MAXN + 1];
    __shared__ long range[2];
    __shared__ int ccount[NCELL];
    const int tid = threadIdx.x, lane = tid & 63;
    const int base = g * nmax;
    if (tid == 0) range[0] = pg_lower_bound(src, E, base);
    if (tid == 1) range[1] = pg_lower_bound(src, E, base + nmax);
    for (int u = tid; u < nmax; u += PG_THREADS) {
        maskL[u] = 0;
        cnt[u] = 0;
    }
    if (tid < NCELL) ccount[tid] = 0;
    __syncthreads();
    const long e0 = range[0];
    const int ne = (int)(range[1] - e0);
    if (tid == 0) eoff[g] = (int)e0;
    if (tid == 0 && g == ngraphs - 1) eoff[ngraphs] = (int)E;
    for (int t = tid; t < ne; t += PG_THREADS) {
        const long e = e0 + t;
        int f[2];
        float fr[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const float v = pseudo[2 * e + d] * 4.0f;
            const float fl = floorf(v);
            f[d] = (int)fl;
            fr[d] = v - fl;
        }
        float b4[4];
        int bits = 0;
        const int gg = f[0] + 5 * f[1];
#pragma unroll
        for (int sidx = 0; sidx < 4; ++sidx) {
            float bb = 1.0f;
            bb = bb * ((sidx & 1) ? fr[0] : 1.0f - fr[0]);
            bb = bb * ((sidx >> 1) ? fr[1] : 1.0f - fr[1]);
            b4[sidx] = bb;
            bits |= 1 << fpm::spline_cell(gg, sidx);
        }
        grp_e[e] = gg;
        *(float4*)(basis_e + 4 * e) = make_float4(b4[0], b4[1], b4[2], b4[3]);
        const int su = src[e] - base;
        atomicOr(&maskL[su], bits);
        atomicAdd(&cnt[dst[e] - base], 1);
    }
    __syncthreads();
    // dst pointers: exclusive scan of the in-degrees (one wave, nmax <= 1024), kept in LDS as the
    // counting-sort cursors
    if (tid < 64) {
        int carry = 0;
        for (int u0 = 0; u0 < nmax; u0 += 64) {
            const int u = u0 + tid;
            const int v = u < nmax ? cnt[u] : 0;
            int incl = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(incl, o);
                if (tid >= o) incl += y;
            }
            if (u < nmax) {
                dst_ptr[base + u] = (int)e0 + carry + incl - v;
                pos[u] = carry + incl - v;
            }
            carry += __shfl(incl, 63);
        }
        if (tid == 0) pos[nmax] = carry;
        if (tid == 0 && g == ngraphs - 1) dst_ptr[(long)ngraphs * nmax] = (int)E;
    }
    __syncthreads();
    // counting sort by destination: (src, edge) keys scattered into each destination's segment
    for (int t = tid; t < ne; t += PG_THREADS) {
        const long e = e0 + t;
        const int slot = atomicAdd(&pos[dst[e] - base], 1);
        key[slot] = ((unsigned)(src[e] - base) << 12) | (unsigned)t;
    }
    // masks (root bit added by the readers, as in the global path) and per-cell node counts
    // (wave ballots, one LDS atomic per wave and cell)
    for (int u0 = 0; u0 < nmax; u0 += PG_THREADS) {
        const int u = u0 + tid;
        const int m = u < nmax ? maskL[u] : 0;
        if (u < nmax) mask[base + u] = m;
        const int mr = u < nmax ? (m | (1 << 25)) : 0;
#pragma unroll
        for (int k = 0; k < NCELL; ++k) {
            const unsigned long long bk = __ballot((mr >> k) & 1);
            if (lane == 0 && bk) atomicAdd(&ccount[k], __popcll(bk));
        }
    }
    __syncthreads();
    // each destination's in-edges ascending by (local source, edge): insertion sort of ~6 keys
    for (int u = tid; u < nmax; u += PG_THREADS) {
        const int end = pos[u], beg = end - cnt[u];
        for (int a = beg + 1; a < end; ++a) {
            const unsigned k = key[a];
            int b = a - 1;
            while (b >= beg && key[b] > k) {
                key[b + 1] = key[b];
                --b;
            }
            key[b + 1] = k;
        }
        for (int a = beg; a < end; ++a) {
            const unsigned k = key[a];
            csr_e[e0 + a] = (int)(e0 + (k & 0xfffu));
            nbr_local[e0 + a] = (int)(k >> 12);
        }
    }
    if (tid < NCELL) cellcnt[g * NCELL + tid] = ccount[tid];
}

__global__ __launch_bounds__(PG_THREADS) void plan_graph_kernel(const int* __restrict__ src,
                                                                const int* __restrict__ dst,
                                                                const float* __restrict__ pseudo, long E, int nmax,
                                                                int ngraphs, int* __restrict__ mask,
                                                                float* __restrict__ basis_e, int* __restrict__ grp_e,
                                                                int* __restrict__ cellcnt, int* __restrict__ dst_ptr,
                                                                int* __restrict__ csr_e, int* __restrict__ nbr_local,
                                                                int* __restrict__ eoff) {
    plan_graph_body(blockIdx.x, src, dst, pseudo, E, nmax, ngraphs, mask, basis_e, grp_e, cellcnt, dst_ptr, csr_e,
                    nbr_local, eoff);
}

// K2: one block -- per-cell exclusive scan over graphs (in place), cell offsets, tile tables
__device__ __forceinline__ void plan_graph_scan_body(int* cellcnt, int ngraphs, int* cell_off, int* tile_info,
                                                     int max_tiles, int* tile_info2, int max_tiles2) {
    __shared__ int cell_tot[NCELL], tile_off[NCELL + 1], coff[NCELL + 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int k = wv; k < NCELL; k += 16) {
        int carry = 0;
        for (int t0 = 0; t0 < ngraphs; t0 += 64) {
            const int i = t0 + lane;
            const int v = i < ngraphs ? cellcnt[i * NCELL + k] : 0;
            int incl = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(incl, o);
                if (lane >= o) incl += y;
            }
            if (i < ngraphs) cellcnt[i * NCELL + k] = carry + incl - v;
            carry += __shfl(incl, 63);
        }
        if (lane == 0) cell_tot[k] = carry;
    }
    __syncthreads();
    if (tid == 0) {
        int off = 0;
        for (int k = 0; k < NCELL; ++k) {
            cell_off[k] = off;
            coff[k] = off;
            off += cell_tot[k];
        }
        cell_off[NCELL] = off;
        coff[NCELL] = off;
    }
    __syncthreads();
    build_tile_table(coff, cell_tot, tile_off, fpm::GBM, tile_info, max_tiles, cell_off + NCELL + 1);
    build_tile_table(coff, cell_tot, tile_off, fpm::G2_BM, tile_info2, max_tiles2, cell_off + NCELL + 2);
}

__global__ __launch_bounds__(1024) void plan_graph_scan_kernel(int* cellcnt, int ngraphs, int* cell_off,
                                                               int* tile_info, int max_tiles, int* tile_info2,
                                                               int max_tiles2) {
    plan_graph_scan_body(cellcnt, ngraphs, cell_off, tile_info, max_tiles, tile_info2, max_tiles2);
}

// K3: rowid / arows (ranks of the graph's nodes per cell, in node order), then the CSR slots'
// 4 product rows and basis weights
__device__ __forceinline__ void plan_graph_rank_body(int g, const int* __restrict__ src, const int* mask, int nmax,
                                                     const int* __restrict__ gbase, const int* __restrict__ cell_off,
                                                     const int* __restrict__ eoff, const int* __restrict__ csr_e,
                                                     const int* __restrict__ grp_e,
                                                     const float* __restrict__ basis_e, int* rowid,
                                                     int* __restrict__ arows, int4* __restrict__ rows4,
                                                     float4* __restrict__ basis4) {
    __shared__ int wc[PG_THREADS / 64][NCELL];
    __shared__ int run[NCELL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long base = (long)g * nmax;
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (tid < NCELL) run[tid] = cell_off[tid] + gbase[g * NCELL + tid];
    __syncthreads();
    for (int u0 = 0; u0 < nmax; u0 += PG_THREADS) {
        const int u = u0 + tid;
        const int m = u < nmax ? (mask[base + u] | (1 << 25)) : 0;
        int myrank[NCELL];
#pragma unroll
        for (int k = 0; k < NCELL; ++k) {
            const unsigned long long b = __ballot((m >> k) & 1);
            if (lane == 0) wc[wave][k] = __popcll(b);
            myrank[k] = __popcll(b & lt);
        }
        __syncthreads();
        if (u < nmax) {
#pragma unroll
            for (int k = 0; k < NCELL; ++k) {
                int r = -1;
                if ((m >> k) & 1) {
                    int pre = run[k];
                    for (int w = 0; w < wave; ++w) pre += wc[w][k];
                    r = pre + myrank[k];
                    arows[r] = (int)(base + u);
                }
                rowid[(base + u) * NCELL + k] = r;
            }
        }
        __syncthreads();
        if (tid < NCELL) {
            int add = 0;
            for (int w = 0; w < PG_THREADS / 64; ++w) add += wc[w][tid];
            run[tid] += add;
        }
        __syncthreads();
    }
    const int e0 = eoff[g], e1 = eoff[g + 1];
    for (int p = e0 + tid; p < e1; p += PG_THREADS) {
        const int e = csr_e[p];
        const int gg = grp_e[e];
        const long sn = src[e];
        int4 r;
        r.x = rowid[sn * NCELL + fpm::spline_cell(gg, 0)];
        r.y = rowid[sn * NCELL + fpm::spline_cell(gg, 1)];
        r.z = rowid[sn * NCELL + fpm::spline_cell(gg, 2)];
        r.w = rowid[sn * NCELL + fpm::spline_cell(gg, 3)];
        rows4[p] = r;
        basis4[p] = *(const float4*)(basis_e + 4 * (long)e);
    }
}

__global__ __launch_bounds__(PG_THREADS) void plan_graph_rank_kernel(const int* __restrict__ src, const int* mask,
                                                                     int nmax, const int* __restrict__ gbase,
                                                                     const int* __restrict__ cell_off,
                                                                     const int* __restrict__ eoff,
                                                                     const int* __restrict__ csr_e,
                                                                     const int* __restrict__ grp_e,
                                                                     const float* __restrict__ basis_e, int* rowid,
                                                                     int* __restrict__ arows, int4* __restrict__ rows4,
                                                                     float4* __restrict__ basis4) {
    plan_graph_rank_body(blockIdx.x, src, mask, nmax, gbase, cell_off, eoff, csr_e, grp_e, basis_e, rowid, arows,
                         rows4, basis4);
}

// Several plans (e.g. every pipeline chunk of one side of a batch) built by one launch of each
// per-graph kernel: job j's graphs are blocks [gstart_j, gstart_j + ngraphs_j) of the K1 / K3
// grids and block j of the K2 grid; job j's plan lives at ws + ws_off_j.  Each plan is the one
// fpm_spline_plan_graphs builds for that job alone (bit-identical).
struct PlanJob {
    const int* src;
    const int* dst;
    const float* pseudo;
    long E, num_nodes, ws_off;
    int ngraphs, gstart;
};

__device__ __forceinline__ int plan_job_of(const PlanJob* __restrict__ jobs, int njobs, int blk) {
    int j = 0;
    while (j + 1 < njobs && jobs[j + 1].gstart <= blk) ++j;
    return j;
}

__global__ __launch_bounds__(PG_THREADS) void plan_multi_graph_kernel(const PlanJob* __restrict__ jobs, int njobs,
                                                                      int nmax, char* ws) {
    const int j = plan_job_of(jobs, njobs, blockIdx.x);
    const PlanJob J = jobs[j];
    const PlanLayout L = plan_layout(J.E, J.num_nodes);
    char* w = ws + J.ws_off;
    plan_graph_body(blockIdx.x - J.gstart, J.src, J.dst, J.pseudo, J.E, nmax, J.ngraphs, (int*)(w + L.mask),
                    (float*)(w + L.basis_e), (int*)(w + L.grp_e), (int*)(w + L.indeg), (int*)(w + L.dst_ptr),
                    (int*)(w + L.csr_e), (int*)(w + L.nbr_local), (int*)(w + L.dslot));
}

__global__ __launch_bounds__(1024) void plan_multi_scan_kernel(const PlanJob* __restrict__ jobs, char* ws) {
    const PlanJob J = jobs[blockIdx.x];
    const PlanLayout L = plan_layout(J.E, J.num_nodes);
    char* w = ws + J.ws_off;
    plan_graph_scan_body((int*)(w + L.indeg), J.ngraphs, (int*)(w + L.cell_off), (int*)(w + L.tile_info),
                         (int)L.max_tiles, (int*)(w + L.tile_info2), (int)L.max_tiles2);
}

__global__ __launch_bounds__(PG_THREADS) void plan_multi_rank_kernel(const PlanJob* __restrict__ jobs, int njobs,
                                                                     int nmax, char* ws) {
    const int j = plan_job_of(jobs, njobs, blockIdx.x);
    const PlanJob J = jobs[j];
    const PlanLayout L = plan_layout(J.E, J.num_nodes);
    char* w = ws + J.ws_off;
    plan_graph_rank_body(blockIdx.x - J.gstart, J.src, (const int*)(w + L.mask), nmax, (const int*)(w + L.indeg),
                         (const int*)(w + L.cell_off), (const int*)(w + L.dslot), (const int*)(w + L.csr_e),
                         (const int*)(w + L.grp_e), (const float*)(w + L.basis_e), (int*)(w + L.rowid),
                         (int*)(w + L.arows), (int4*)(w + L.rows4), (float4*)(w + L.basis4));
}

// out[v] = max_{in-edges e} sum_s basis[e,s] * Y[row(src_e, cell_s)] + Y[root row v] + bias
//   mode & 1 == 0: relu(.) ; mode & 1 == 1: xres[v] + 0.1 * (.)   (+ optional per-pair column scale
//   on out_t).  mode >> 1 (bf16 out_t only): the operand rows are written split for a near-fp32
//   product on the bf16 MFMA path, 3 x 768 columns per row (hi = bf16(z), lo = bf16(z - hi)):
//   1 = [hi | lo | hi] (the A operand), 2 = [hi | hi | lo] (the B operand) -- A . B over the 2304
//   columns is hi.hi + lo.hi + hi.lo, exactly fpm_split_bf16x3's x [W_hi | W_hi | W_lo] pairing.
// One wave per node, 12 channels per lane: 8 contiguous at 8 lane (one 16-B bf16 load per product
// row) + 4 at 512 + 4 lane (comb_chan).  (An in-edge prefetch variant -- row ids in lanes, two
// edges' 8 product rows in flight -- measured neutral and was dropped.)
// ARG (training forward): also record, per (node, channel), the CSR slot of the in-edge attaining
// the max (the first one in CSR order, -1 without in-edges) for the scatter backward.
__device__ __forceinline__ int comb_chan(int lane, int t) { return t < 2 ? 8 * lane + 4 * t : 512 + 4 * lane; }

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

template <typename T, int NPB = 4, bool ARG = false, int SPOL = 0>
__global__ __launch_bounds__(64 * NPB) void combine_kernel(const T* __restrict__ Y, const int* __restrict__ cell_off,
                                                      const float* __restrict__ bias,
                                                      const int* __restrict__ dst_ptr, const int4* __restrict__ rows4,
                                                      const float4* __restrict__ basis4, long num_nodes, int nmax,
                                                      const int* __restrict__ nvalid, int mode,
                                                      const float* __restrict__ xres, const float* __restrict__ cscale,
                                                      float* __restrict__ out_f, T* __restrict__ out_t,
                                                      int* __restrict__ argmax = nullptr) {
    const int lane = threadIdx.x & 63;
    // graph-per-XCD block order: XCD x = blockIdx % 8 takes graphs x, x+8, ... so a graph's product
    // rows (~3.7 MB at n = 256, each read ~2.4 times by its in-edges) stay in one L2
    const int bpg = (nmax + NPB - 1) / NPB;
    const int xk = blockIdx.x >> 3;
    const int b = (xk / bpg) * 8 + (blockIdx.x & 7);
    const int loc = (xk % bpg) * NPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (loc >= nmax || (long)b * nmax >= num_nodes) return;
    const long v = (long)b * nmax + loc;
    const bool valid = loc < nvalid[b];
    const int beg = dst_ptr[v], end = dst_ptr[v + 1];
    const long root_row = (long)cell_off[25] + v;
    float m[3][4];
    int am[3][4];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m[t][j] = beg < end ? -INFINITY : 0.f;   // torch_scatter: empty -> 0
            am[t][j] = -1;
        }
    (void)am;
    for (int e = beg; e < end; ++e) {
        const int4 r = rows4[e];
        const float4 bs = basis4[e];
        // 16-B aligned rows (768 channels): lets the two 8-B loads of t = 0, 1 merge into one
        const T* y0 = (const T*)__builtin_assume_aligned(Y + (long)r.x * 768, 16);
        const T* y1 = (const T*)__builtin_assume_aligned(Y + (long)r.y * 768, 16);
        const T* y2 = (const T*)__builtin_assume_aligned(Y + (long)r.z * 768, 16);
        const T* y3 = (const T*)__builtin_assume_aligned(Y + (long)r.w * 768, 16);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int c0 = comb_chan(lane, t);
            float a0[4], a1[4], a2[4], a3[4];
            fpm::load4(y0 + c0, a0);
            fpm::load4(y1 + c0, a1);
            fpm::load4(y2 + c0, a2);
            fpm::load4(y3 + c0, a3);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float msg = bs.x * a0[j];
                msg = fmaf(bs.y, a1[j], msg);
                msg = fmaf(bs.z, a2[j], msg);
                msg = fmaf(bs.w, a3[j], msg);
                if constexpr (ARG) {
                    if (msg > m[t][j]) am[t][j] = e;    // strict: the first maximum in CSR order
                }
                m[t][j] = fmaxf(m[t][j], msg);
            }
        }
    }
    if constexpr (ARG) {
#pragma unroll
        for (int t = 0; t < 3; ++t)
            *(int4*)(argmax + v * 768 + comb_chan(lane, t)) = make_int4(am[t][0], am[t][1], am[t][2], am[t][3]);
    }
    const T* yr = (const T*)__builtin_assume_aligned(Y + root_row * 768, 16);
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int c0 = comb_chan(lane, t);
        float rt[4], bi[4], xr[4] = {0.f, 0.f, 0.f, 0.f};
        fpm::load4(yr + c0, rt);
        fpm::load4(bias + c0, bi);                       // 16-B vector loads (rows are 3 KB aligned)
        if (mode & 1) fpm::load4(xres + v * 768 + c0, xr);
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float o = (m[t][j] + rt[j]) + bi[j];
            if (!(mode & 1)) y[j] = fmaxf(o, 0.f);
            else y[j] = xr[j] + 0.1f * o;
            if (!valid) y[j] = 0.f;
        }
        // SPOL = 16 (sc1): the output lines leave the XCD's L2 rather than evicting the product rows
        // the other in-flight nodes still gather (the next layer reads these rows much later)
        if (out_f) {
            if constexpr (SPOL != 0) {
                const __amdgpu_buffer_rsrc_t rf =
                    __builtin_amdgcn_make_buffer_rsrc((void*)(out_f + v * 768), (short)0, 768 * 4, 0x00020000);
                const u32x4_t pk = {__float_as_uint(y[0]), __float_as_uint(y[1]), __float_as_uint(y[2]),
                                    __float_as_uint(y[3])};
                __builtin_amdgcn_raw_buffer_store_b128(pk, rf, c0 * 4, 0, SPOL);
            } else {
                *(float4*)(out_f + v * 768 + c0) = make_float4(y[0], y[1], y[2], y[3]);
            }
        }
        if (out_t) {
            float z[4] = {y[0], y[1], y[2], y[3]};
            if (cscale) {
                float cs[4];
                fpm::load4(cscale + (long)b * 768 + c0, cs);
#pragma unroll
                for (int j = 0; j < 4; ++j) z[j] = y[j] * cs[j];
            }
            const int split = mode >> 1;
            if (sizeof(T) == 2 && split) {
                float lo[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) lo[j] = z[j] - fpm::to_f<T>(fpm::from_f<T>(z[j]));
                T* o3 = out_t + v * 2304 + c0;
                fpm::store4(o3, z);
                fpm::store4(o3 + 768, split == 1 ? lo : z);
                fpm::store4(o3 + 1536, split == 1 ? z : lo);
            } else if constexpr (SPOL != 0) {
                const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(
                    (void*)(out_t + v * 768), (short)0, (int)(768 * sizeof(T)), 0x00020000);
                if constexpr (sizeof(T) == 2) {
                    const u32x2_t pk = {(uint32_t)fpm::from_f<T>(z[0]) | ((uint32_t)fpm::from_f<T>(z[1]) << 16),
                                        (uint32_t)fpm::from_f<T>(z[2]) | ((uint32_t)fpm::from_f<T>(z[3]) << 16)};
                    __builtin_amdgcn_raw_buffer_store_b64(pk, rt, c0 * 2, 0, SPOL);
                } else {
                    const u32x4_t pk = {__float_as_uint(z[0]), __float_as_uint(z[1]), __float_as_uint(z[2]),
                                        __float_as_uint(z[3])};
                    __builtin_amdgcn_raw_buffer_store_b128(pk, rt, c0 * 4, 0, SPOL);
                }
            } else {
                fpm::store4(out_t + v * 768 + c0, z);
            }
        }
    }
}


// ---- training backward -------------------------------------------------
// Gradient of one SplineConv layer w.r.t. its product rows:  with g the gradient of the layer's
// pre-activation (mode 0: gout * [out > 0], the F.relu; mode 1: 0.1 * gout, the Siamese residual
// scale), the max over in-edges routes g[v, c] to the in-edge e* attaining the max (the first one
// in the deterministic CSR order; messages are recomputed exactly as the forward did), i.e.
// dY[row(src e*, cell_s)] += basis_s * g, and the root product row of v receives g itself.
// Several destinations share a (source, cell) row, so those adds are fp32 atomics.
template <typename T>
__global__ __launch_bounds__(256) void combine_bwd_kernel(const T* __restrict__ Y, const int* __restrict__ cell_off,
                                                          const int* __restrict__ dst_ptr,
                                                          const int4* __restrict__ rows4,
                                                          const float4* __restrict__ basis4, long num_nodes, int nmax,
                                                          const int* __restrict__ nvalid, int mode,
                                                          const float* __restrict__ gout,
                                                          const float* __restrict__ hout, float* __restrict__ dY) {
    const int lane = threadIdx.x & 63;
    const long v = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= num_nodes) return;
    const int b = (int)(v / nmax), loc = (int)(v - (long)b * nmax);
    const bool valid = loc < nvalid[b];
    const int beg = dst_ptr[v], end = dst_ptr[v + 1];
    const long root_row = (long)cell_off[25] + v;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int c0 = 4 * lane + 256 * t;
        float g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gv = valid ? gout[v * 768 + c0 + j] : 0.f;
            if (mode == 0) gv = (valid && hout[v * 768 + c0 + j] > 0.f) ? gv : 0.f;
            else gv *= 0.1f;
            g[j] = gv;
        }
        *(float4*)(dY + root_row * 768 + c0) = make_float4(g[0], g[1], g[2], g[3]);
        if (beg >= end) continue;
        float m[4];
        int am[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { m[j] = -INFINITY; am[j] = beg; }
        for (int e = beg; e < end; ++e) {
            const int4 r = rows4[e];
            const float4 bs = basis4[e];
            float a0[4], a1[4], a2[4], a3[4];
            fpm::load4(Y + (long)r.x * 768 + c0, a0);
            fpm::load4(Y + (long)r.y * 768 + c0, a1);
            fpm::load4(Y + (long)r.z * 768 + c0, a2);
            fpm::load4(Y + (long)r.w * 768 + c0, a3);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float msg = bs.x * a0[j];
                msg = fmaf(bs.y, a1[j], msg);
                msg = fmaf(bs.z, a2[j], msg);
                msg = fmaf(bs.w, a3[j], msg);
                if (msg > m[j]) { m[j] = msg; am[j] = e; }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (g[j] == 0.f) continue;
            const int4 r = rows4[am[j]];
            const float4 bs = basis4[am[j]];
            unsafeAtomicAdd(dY + (long)r.x * 768 + c0 + j, bs.x * g[j]);
            unsafeAtomicAdd(dY + (long)r.y * 768 + c0 + j, bs.y * g[j]);
            unsafeAtomicAdd(dY + (long)r.z * 768 + c0 + j, bs.z * g[j]);
            unsafeAtomicAdd(dY + (long)r.w * 768 + c0 + j, bs.w * g[j]);
        }
    }
}

// Scatter form of the same gradient without atomics (training forward recorded the argmax slots):
// one 768-thread workgroup per SOURCE node u, thread = channel c; walking u's out-edges e = (u, v)
// in a fixed order (the reversed plan's CSR), the slot p of e in v's in-edge list gets
// dY[row(u, cell_s(e))][c] += basis_s(e) * g[v][c] wherever argmax[v][c] == p.  Accumulators are
// LDS rows acc[cell][c] (each thread owns its channel column: no barriers, no bank conflicts);
// every product row of u is written once (no memset), and the root row of u gets g[u].
// Deterministic.  slot_of[e] = the CSR slot of edge e (fpm_spline_slot_of).
// f32_rows == 0 (with dYb): the cell rows go to the bf16 operand copy only (the weight-gradient and
// dX products read that copy; the fp32 rows' one reader is the bias gradient, i.e. the root rows),
// which drops 2/3 of the kernel's HBM writes.
// QB: out-edges per batch -- the batch's index loads (uniform) and its argmax / gout / hout loads
// are all issued before any of its LDS updates, which then run in the same edge order as QB = 1
// (bit-identical; QB = 1 waits on one edge's loads at a time).
template <int QB>
__global__ __launch_bounds__(768) void combine_scatter_bwd_kernel(
    const int* __restrict__ cell_off, const int* __restrict__ rowid, const int* __restrict__ mask,
    const int* __restrict__ grp_e, const float* __restrict__ basis_e, const int* __restrict__ rptr,
    const int* __restrict__ rcsr_e, const int* __restrict__ rnbr, const int* __restrict__ slot_of,
    const int* __restrict__ argmax, long num_nodes, int nmax, const int* __restrict__ nvalid, int mode,
    const float* __restrict__ gout, const float* __restrict__ hout, float* __restrict__ dY,
    bf16_t* __restrict__ dYb, int f32_rows) {
    // dYb (bf16 mode): the same rows' bf16 operand copy for the dX product GEMM, written here
    // instead of a separate cast pass over the plan's row bound (~2.5x the real rows)
    extern __shared__ float acc[];                       // [NCELL - 1][768]
    const long u = blockIdx.x;
    const int c = threadIdx.x;
    const int b = (int)(u / nmax);
    const long base = (long)b * nmax;
    const int nvb = nvalid[b];
    auto gsel = [&](bool valid, float g, float h) -> float {
        if (!valid) return 0.f;
        return mode == 0 ? (h > 0.f ? g : 0.f) : 0.1f * g;
    };
    const int m = mask[u];
    for (int k = 0; k < NCELL - 1; ++k)
        if ((m >> k) & 1) acc[k * 768 + c] = 0.f;
    const int q0 = rptr[u], q1 = rptr[u + 1];
    for (int qb = q0; qb < q1; qb += QB) {
        int ee[QB], pe[QB], am[QB];
        bool vv[QB];
        float gv[QB], hv[QB];
#pragma unroll
        for (int i = 0; i < QB; ++i) {
            const int q = min(qb + i, q1 - 1);            // past the end: a repeat, skipped below
            ee[i] = rcsr_e[q];
            const int vl = rnbr[q];
            const long v = base + vl;
            pe[i] = slot_of[ee[i]];
            vv[i] = vl < nvb;
            am[i] = argmax[v * 768 + c];
            gv[i] = gout[v * 768 + c];
            hv[i] = mode == 0 ? hout[v * 768 + c] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < QB; ++i) {
            if (qb + i >= q1 || am[i] != pe[i]) continue;
            const float g = gsel(vv[i], gv[i], hv[i]);
            const int gg = grp_e[ee[i]];
            const float4 bs = *(const float4*)(basis_e + 4 * (long)ee[i]);
            acc[fpm::spline_cell(gg, 0) * 768 + c] += bs.x * g;
            acc[fpm::spline_cell(gg, 1) * 768 + c] += bs.y * g;
            acc[fpm::spline_cell(gg, 2) * 768 + c] += bs.z * g;
            acc[fpm::spline_cell(gg, 3) * 768 + c] += bs.w * g;
        }
    }
    for (int k = 0; k < NCELL - 1; ++k)
        if ((m >> k) & 1) {
            const long o = (long)rowid[u * NCELL + k] * 768 + c;
            if (f32_rows) dY[o] = acc[k * 768 + c];
            if (dYb) dYb[o] = fpm::f2bf(acc[k * 768 + c]);
        }
    const long o = ((long)cell_off[NCELL - 1] + u) * 768 + c;
    const float gu = gsel((int)(u - base) < nvb, gout[u * 768 + c], mode == 0 ? hout[u * 768 + c] : 0.f);
    dY[o] = gu;
    if (dYb) dYb[o] = fpm::f2bf(gu);
}

// out[c][q] = rows[q] >= 0 ? in[rows[q]][c] : 0 for c < C, q < Q (ldo >= Q): the K-major operand
// copies of the per-cell weight-gradient GEMMs (dW_cell = X_rows^T dY_rows as A B^T with
// K = rows).  64 x 64 tiles through LDS (padded rows: conflict-free column reads).
__global__ __launch_bounds__(256) void gather_transpose_f32_kernel(const float* __restrict__ in, long ldi,
                                                                   const int* __restrict__ rows, long Q, int C,
                                                                   float* __restrict__ out, long ldo) {
    __shared__ float tile[64][65];
    const long q0 = (long)blockIdx.x * 64;
    const int c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int k = ty; k < 64; k += 4) {
        const long q = q0 + k;
        const int r = q < Q ? rows[q] : -1;
        float v = 0.f;
        if (r >= 0 && c0 + tx < C) v = in[(long)r * ldi + c0 + tx];
        tile[k][tx] = v;
    }
    __syncthreads();
    for (int k = ty; k < 64; k += 4) {
        const int c = c0 + k;
        if (c < C && q0 + tx < Q) out[(long)c * ldo + q0 + tx] = tile[tx][k];
    }
}

// bf16: 32-bit global accesses on both sides (a channel pair per load, a row pair per store);
// C % 64 == 0, Q % 2 == 0 and ldo even (the caller's padded chunks)
__global__ __launch_bounds__(256) void gather_transpose_bf16_kernel(const bf16_t* __restrict__ in, long ldi,
                                                                    const int* __restrict__ rows, long Q, int C,
                                                                    bf16_t* __restrict__ out, long ldo) {
    __shared__ uint32_t tile[64][33];                       // [q][channel pair]
    const long q0 = (long)blockIdx.x * 64;
    const int c0 = blockIdx.y * 64;
    const int t = threadIdx.x, cp = t & 31, ry = t >> 5;    // 8 rows per pass
    for (int k = ry; k < 64; k += 8) {
        const long q = q0 + k;
        const int r = q < Q ? rows[q] : -1;
        uint32_t v = 0u;
        if (r >= 0) v = *(const uint32_t*)(in + (long)r * ldi + c0 + 2 * cp);
        tile[k][cp] = v;
    }
    __syncthreads();
    const int qp = t & 31, cy = t >> 5;                     // 32 row pairs x 8 channels per pass
    const bf16_t* T = (const bf16_t*)&tile[0][0];           // [q][66] halfwords
    for (int c = cy; c < 64; c += 8) {
        const long q = q0 + 2 * qp;
        if (q >= Q) continue;
        const uint32_t lo = T[(2 * qp) * 66 + c], hi = T[(2 * qp + 1) * 66 + c];
        *(uint32_t*)(out + (long)(c0 + c) * ldo + q) = lo | (hi << 16);
    }
}

// bf16 on 16-B global accesses: 8 channels per load, 8 rows per store (C % 64 == 0, Q, ldi, ldo
// multiples of 8, 16-B aligned buffers); LDS rows of 68 halfwords (8-B aligned writes, rows of a
// store's 8-row gather spread over the banks)
__global__ __launch_bounds__(256) void gather_transpose_bf16x8_kernel(const bf16_t* __restrict__ in, long ldi,
                                                                      const int* __restrict__ rows, long Q, int C,
                                                                      bf16_t* __restrict__ out, long ldo) {
    constexpr int LD = 68;
    __shared__ __attribute__((aligned(16))) bf16_t tile[64 * LD];   // [q][c]
    const long q0 = (long)blockIdx.x * 64;
    const int c0 = blockIdx.y * 64, t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = t + 256 * i, k = idx >> 3, ch = idx & 7;
        const long q = q0 + k;
        const int r = q < Q ? rows[q] : -1;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (r >= 0) v = *(const uint4*)(in + (long)r * ldi + c0 + ch * 8);
        uint2* d = (uint2*)(tile + k * LD + ch * 8);
        d[0] = make_uint2(v.x, v.y);
        d[1] = make_uint2(v.z, v.w);
    }
    __syncthreads();
    const unsigned short* T = (const unsigned short*)tile;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = t + 256 * i, c = idx >> 3, qc = idx & 7;
        const long q = q0 + qc * 8;
        if (q >= Q) continue;
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            w[j] = (uint32_t)T[(qc * 8 + 2 * j) * LD + c] | ((uint32_t)T[(qc * 8 + 2 * j + 1) * LD + c] << 16);
        *(uint4*)(out + (long)(c0 + c) * ldo + q) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

__global__ void slot_of_kernel(const int* __restrict__ csr_e, long E, int* __restrict__ slot_of) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < E) slot_of[csr_e[p]] = (int)p;
}

// dX[u] (+)= sum over u's product rows (cells in ascending order, then the root) of dXrows[row]:
// the transpose of the forward's row gather, in a fixed order (no atomics).
__global__ __launch_bounds__(256) void node_rows_sum_kernel(const float* __restrict__ dXrows,
                                                            const int* __restrict__ rowid, long num_nodes,
                                                            int accumulate, float* __restrict__ dX) {
    const long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (u >= num_nodes) return;
    float acc[3][4];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = 0.f;
    for (int k = 0; k < NCELL; ++k) {
        const int r = rowid[u * NCELL + k];
        if (r < 0) continue;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            float a[4];
            fpm::load4(dXrows + (long)r * 768 + 4 * lane + 256 * t, a);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[t][j] += a[j];
        }
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        float* o = dX + u * 768 + 4 * lane + 256 * t;
        if (accumulate) {
            float p[4];
            fpm::load4(o, p);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[t][j] += p[j];
        }
        fpm::store4(o, acc[t]);
    }
}

}  // namespace

// destination nodes (one wave each) per combine workgroup: 4, 8 or 16 (bit-identical); env
// FPM_GEMM_SC1 or fpm_set_tuning("gemm_store_sc1", v): the product GEMM's bf16 output tiles stored
// with the sc1 cache policy (1) or plain (0, default: sc1 measured 3 % slower alone, 0.341 vs 0.331 ms)
int& gemm_store_sc1_flag() {
    static int v = [] {
        const char* e = getenv("FPM_GEMM_SC1");
        return e ? atoi(e) : 0;
    }();
    return v;
}

// FPM_COMBINE_SC1 or fpm_set_tuning("combine_store_sc1", v): the combine's output stores with the
// sc1 cache policy (1) or plain (0, default: neutral end to end, profiles/r04e_sc1_ab.txt)
int& combine_store_sc1_flag() {
    static int v = [] {
        const char* e = getenv("FPM_COMBINE_SC1");
        return e ? atoi(e) : 0;
    }();
    return v;
}

// fpm_set_tuning("combine_lds_kb", v): dynamic LDS reserved per combine workgroup (0 default); a
// residency cap (160 / v workgroups per CU) so fewer graphs' product rows are live per XCD L2 (A/B)
int& combine_lds_kb_flag() {
    static int v = 0;
    return v;
}

// FPM_COMBINE_NPB or fpm_set_tuning("combine_npb", v)
int& combine_npb_flag() {
    static int u = [] {
        const char* e = getenv("FPM_COMBINE_NPB");
        return e ? atoi(e) : 4;
    }();
    return u;
}

extern "C" long fpm_spline_plan_bytes(long E, long num_nodes) {
    return plan_layout(E, num_nodes).total;
}

// Product-row workspace of fpm_spline_conv_fwd: max_rows x 768 operand-dtype values.
extern "C" long fpm_spline_y_bytes(int dtype, long E, long num_nodes) {
    return plan_max_rows(E, num_nodes) * 768L * (dtype == 0 ? 4 : 2);
}

extern "C" int fpm_spline_plan(const int* src, const int* dst, const float* pseudo, long E, long num_nodes, int nmax,
                               void* ws, long ws_bytes, void* stream) {
    PlanLayout L = plan_layout(E, num_nodes);
    FPM_CHECK_ARG(ws_bytes >= L.total, "spline_plan: workspace too small");
    FPM_CHECK_ARG(E > 0 && num_nodes > 0 && nmax > 0, "spline_plan: bad sizes");
    FPM_CHECK_ARG(num_nodes * NCELL < (1L << 31) && L.max_rows < (1L << 31), "spline_plan: batch too large");
    char* w = (char*)ws;
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(w + L.mask, 0, num_nodes * 4, st);
    (void)hipMemsetAsync(w + L.indeg, 0, num_nodes * 4, st);
    const unsigned eblocks = (unsigned)((E + 255) / 256);
    const unsigned nblocks = (unsigned)L.nblk;
    hipLaunchKernelGGL(plan_edge_kernel, dim3(eblocks), dim3(256), 0, st, src, dst, pseudo, E, (int*)(w + L.mask),
                       (int*)(w + L.indeg), (int*)(w + L.dslot), (float*)(w + L.basis_e), (int*)(w + L.grp_e));
    hipLaunchKernelGGL(plan_blkcount_kernel, dim3(nblocks), dim3(256), 0, st, (const int*)(w + L.mask), num_nodes,
                       (int*)(w + L.blk_cnt));
    hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(1024), 0, st, (int*)(w + L.blk_cnt), L.nblk,
                       (int*)(w + L.cell_off), (int*)(w + L.tile_info), (int)L.max_tiles, (int*)(w + L.tile_info2),
                       (int)L.max_tiles2, (const int*)(w + L.indeg), (int*)(w + L.dst_ptr), num_nodes);
    hipLaunchKernelGGL(plan_rank_kernel, dim3(nblocks), dim3(256), 0, st, (const int*)(w + L.mask), num_nodes,
                       (const int*)(w + L.blk_cnt), (const int*)(w + L.cell_off), (int*)(w + L.rowid),
                       (int*)(w + L.arows));
    hipLaunchKernelGGL(plan_fill_kernel, dim3(eblocks), dim3(256), 0, st, src, dst, E, nmax,
                       (const int*)(w + L.dslot), (const int*)(w + L.dst_ptr), (int*)(w + L.csr_e),
                       (int*)(w + L.nbr_local));
    hipLaunchKernelGGL(plan_sort_kernel, dim3((unsigned)((num_nodes + 255) / 256)), dim3(256), 0, st,
                       (const int*)(w + L.dst_ptr), num_nodes, (int*)(w + L.csr_e), (int*)(w + L.nbr_local));
    hipLaunchKernelGGL(plan_expand_kernel, dim3(eblocks), dim3(256), 0, st, src, (const int*)(w + L.csr_e), E,
                       (const int*)(w + L.grp_e), (const float*)(w + L.basis_e), (const int*)(w + L.rowid),
                       (int4*)(w + L.rows4), (float4*)(w + L.basis4));
    return fpm::check_launch("fpm_spline_plan");
}

// K-major gather-transpose for the per-cell weight-gradient GEMMs (training): dtype 0 fp32, 1 bf16
extern "C" int fpm_gather_transpose(int dtype, const void* in, long ldi, const int* rows, long Q, int C, void* out,
                                    long ldo, void* stream) {
    FPM_CHECK_ARG((dtype == 0 || dtype == 1) && Q >= 0 && C > 0 && ldo >= Q, "gather_transpose: bad args");
    if (Q == 0) return 0;
    const dim3 grid((unsigned)((Q + 63) / 64), (unsigned)((C + 63) / 64));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0) {
        hipLaunchKernelGGL(gather_transpose_f32_kernel, grid, dim3(256), 0, st, (const float*)in, ldi, rows, Q, C,
                           (float*)out, ldo);
    } else {
        FPM_CHECK_ARG(C % 64 == 0 && Q % 2 == 0 && ldo % 2 == 0 && ldi % 2 == 0 && ((uintptr_t)in & 3) == 0 &&
                          ((uintptr_t)out & 3) == 0,
                      "gather_transpose: bf16 needs C %% 64 == 0, even Q / ldo / ldi, 4-B aligned buffers");
        if (Q % 8 == 0 && ldo % 8 == 0 && ldi % 8 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0)
            hipLaunchKernelGGL(gather_transpose_bf16x8_kernel, grid, dim3(256), 0, st, (const bf16_t*)in, ldi, rows, Q,
                               C, (bf16_t*)out, ldo);
        else
            hipLaunchKernelGGL(gather_transpose_bf16_kernel, grid, dim3(256), 0, st, (const bf16_t*)in, ldi, rows, Q, C,
                               (bf16_t*)out, ldo);
    }
    return fpm::check_launch("fpm_gather_transpose");
}

// Per-graph plan when every graph has <= 4096 edges and nmax <= 1024 (max_graph_edges: the
// caller's bound, e.g. from the batch's host edge offsets); otherwise the global kernels.  The
// scratch fields blk_cnt (per-graph cell counts / bases) and dslot (graph edge offsets) are reused.
// per-graph plan kernels (1, default) or the global ones (0); bit-identical.  Env FPM_PLAN_GRAPH or
// fpm_set_tuning("plan_graph", v)
int& plan_graph_flag() {
    static int v = [] {
        const char* e = getenv("FPM_PLAN_GRAPH");
        return e ? atoi(e) : 1;
    }();
    return v;
}

extern "C" int fpm_spline_plan_graphs(const int* src, const int* dst, const float* pseudo, long E, long num_nodes,
                                      int nmax, long max_graph_edges, void* ws, long ws_bytes, void* stream) {
    const long ngraphs = nmax > 0 ? num_nodes / nmax : 0;
    // the per-graph path keeps its per-graph cell counts in the indeg scratch (num_nodes ints) and
    // the graph edge offsets in the dslot scratch (E ints)
    const bool fits = max_graph_edges > 0 && max_graph_edges <= PG_MAXE && nmax <= PG_MAXN && nmax >= NCELL &&
                      ngraphs > 0 && ngraphs * nmax == num_nodes && ngraphs + 1 <= E;
    if (!fits || plan_graph_flag() == 0)
        return fpm_spline_plan(src, dst, pseudo, E, num_nodes, nmax, ws, ws_bytes, stream);
    PlanLayout L = plan_layout(E, num_nodes);
    FPM_CHECK_ARG(ws_bytes >= L.total, "spline_plan: workspace too small");
    FPM_CHECK_ARG(num_nodes * NCELL < (1L << 31) && L.max_rows < (1L << 31), "spline_plan: batch too large");
    char* w = (char*)ws;
    hipStream_t st = (hipStream_t)stream;
    int* gcnt = (int*)(w + L.indeg);
    int* eoff = (int*)(w + L.dslot);
    hipLaunchKernelGGL(plan_graph_kernel, dim3((unsigned)ngraphs), dim3(PG_THREADS), 0, st, src, dst, pseudo, E, nmax,
                       (int)ngraphs, (int*)(w + L.mask), (float*)(w + L.basis_e), (int*)(w + L.grp_e), gcnt,
                       (int*)(w + L.dst_ptr), (int*)(w + L.csr_e), (int*)(w + L.nbr_local), eoff);
    hipLaunchKernelGGL(plan_graph_scan_kernel, dim3(1), dim3(1024), 0, st, gcnt, (int)ngraphs, (int*)(w + L.cell_off),
                       (int*)(w + L.tile_info), (int)L.max_tiles, (int*)(w + L.tile_info2), (int)L.max_tiles2);
    hipLaunchKernelGGL(plan_graph_rank_kernel, dim3((unsigned)ngraphs), dim3(PG_THREADS), 0, st, src,
                       (const int*)(w + L.mask), nmax, (const int*)gcnt, (const int*)(w + L.cell_off),
                       (const int*)eoff, (const int*)(w + L.csr_e), (const int*)(w + L.grp_e),
                       (const float*)(w + L.basis_e), (int*)(w + L.rowid), (int*)(w + L.arows), (int4*)(w + L.rows4),
                       (float4*)(w + L.basis4));
    return fpm::check_launch("fpm_spline_plan_graphs");
}

// jobs: device array of njobs PlanJob (host-built: each job's inputs, sizes, first block and
// 256-aligned offset into ws, where job j's plan needs fpm_spline_plan_bytes(E_j, nodes_j));
// every job must satisfy the per-graph conditions of fpm_spline_plan_graphs (checked by the
// caller: graphs of <= 4096 edges, 26 <= nmax <= 1024, num_nodes = ngraphs * nmax).
extern "C" int fpm_spline_plan_multi(const void* jobs, int njobs, int total_graphs, int nmax, void* ws, void* stream) {
    FPM_CHECK_ARG(njobs >= 1 && total_graphs >= njobs, "spline_plan_multi: bad job count");
    FPM_CHECK_ARG(nmax >= NCELL && nmax <= PG_MAXN, "spline_plan_multi: nmax must be in [%d, %d]", NCELL, PG_MAXN);
    hipStream_t st = (hipStream_t)stream;
    const PlanJob* J = (const PlanJob*)jobs;
    hipLaunchKernelGGL(plan_multi_graph_kernel, dim3((unsigned)total_graphs), dim3(PG_THREADS), 0, st, J, njobs, nmax,
                       (char*)ws);
    hipLaunchKernelGGL(plan_multi_scan_kernel, dim3((unsigned)njobs), dim3(1024), 0, st, J, (char*)ws);
    hipLaunchKernelGGL(plan_multi_rank_kernel, dim3((unsigned)total_graphs), dim3(PG_THREADS), 0, st, J, njobs, nmax,
                       (char*)ws);
    return fpm::check_launch("fpm_spline_plan_multi");
}

extern "C" int fpm_spline_plan_job_bytes(void) { return (int)sizeof(PlanJob); }

// Pointers into the plan for the GNN layer (dst CSR with local neighbour indices).
extern "C" int fpm_spline_plan_csr(void* ws, long E, long num_nodes, int** dst_ptr, int** nbr_local) {
    PlanLayout L = plan_layout(E, num_nodes);
    *dst_ptr = (int*)((char*)ws + L.dst_ptr);
    *nbr_local = (int*)((char*)ws + L.nbr_local);
    return 0;
}

// One SplineConv layer over a whole side-batch.
//   mode 0: out = relu(max_e msg + x R + b)            (conv 0 + F.relu, spline_conv.py:35)
//   mode 1: out = xres + 0.1 * (max_e msg + x R + b)   (conv 1 + Siamese residual, :38, :56)
// x_op: operand copy of the input (dtype); W: (26, 768 out, 768 in) = the 25 spline cells then the
// root weight transposed.  y_ws: fpm_spline_y_bytes bytes.  cscale (B,768) optionally scales the
// operand output (X o c for the vertex affinity, affinity_layer.py:15).
extern "C" int fpm_spline_conv_fwd_argmax(int dtype, const void* x_op, const void* plan_ws, long E, long num_nodes,
                                          int nmax, const int* nvalid, const void* W, const float* bias, void* y_ws,
                                          long y_ws_bytes, int mode, const float* xres, const float* cscale,
                                          float* out_f, void* out_t, int* argmax, void* stream);

extern "C" int fpm_spline_conv_fwd(int dtype, const void* x_op, const void* plan_ws, long E, long num_nodes, int nmax,
                                   const int* nvalid, const void* W, const float* bias, void* y_ws, long y_ws_bytes,
                                   int mode, const float* xres, const float* cscale, float* out_f, void* out_t,
                                   void* stream) {
    return fpm_spline_conv_fwd_argmax(dtype, x_op, plan_ws, E, num_nodes, nmax, nvalid, W, bias, y_ws, y_ws_bytes, mode,
                                      xres, cscale, out_f, out_t, nullptr, stream);
}

// the same, also writing argmax[num_nodes][768] (int32 CSR slot of each channel's max in-edge, -1
// without in-edges) when argmax != nullptr -- the training forward, for the scatter backward
extern "C" int fpm_spline_conv_fwd_argmax(int dtype, const void* x_op, const void* plan_ws, long E, long num_nodes,
                                          int nmax, const int* nvalid, const void* W, const float* bias, void* y_ws,
                                          long y_ws_bytes, int mode, const float* xres, const float* cscale,
                                          float* out_f, void* out_t, int* argmax, void* stream) {
    using namespace fpm;
    FPM_CHECK_ARG(dtype == 0 || dtype == 1, "spline_conv: bad dtype");
    FPM_CHECK_ARG(mode >= 0 && mode <= 5 && (!(mode & 1) || xres), "spline_conv: mode %d: bit 0 (residual) needs xres, "
                  "mode >> 1 must be 0, 1 or 2", mode);
    FPM_CHECK_ARG(!(mode >> 1) || (dtype == 1 && out_t && !argmax),
                  "spline_conv: split operand rows (mode >> 1) need bf16 out_t (inference forward)");
    FPM_CHECK_ARG(y_ws_bytes >= fpm_spline_y_bytes(dtype, E, num_nodes), "spline_conv: y workspace too small");
    PlanLayout L = plan_layout(E, num_nodes);
    const char* w = (const char*)plan_ws;
    hipStream_t st = (hipStream_t)stream;
    const int D = 768;
    // all (node, cell) products in one grouped GEMM (group = cell, B = that cell's weight)
    {
        GemmParams p = {};
        p.A = x_op; p.lda = D; p.a_rows = (const int*)(w + L.arows);
        p.B = W; p.ldb = D; p.sB_seg = (long)D * D;
        p.M = (int)L.max_rows; p.N = D; p.K = D; p.nseg = 1;
        p.tile_info = (const int*)(w + L.tile_info);
        p.group_off = (const int*)(w + L.cell_off);
        p.epi = EPI_STORE; p.ldc = D;
        if (dtype == 0) p.Cf = (float*)y_ws;
        else p.Ct = y_ws;
        p.store_sc1 = gemm_store_sc1_flag();
        p.remap_mtiles = (int)(dtype == 0 ? L.max_tiles : L.max_tiles2);
        if (dtype == 1) p.tile_info = (const int*)(w + L.tile_info2);
        // bf16: the walk kernel (gemm_phase.h; S row tiles per workgroup, forced or picked by the kernel
        // from the plan's real tile count), 0 = the phase kernel
        const int walk = dtype == 1 ? gemm_walk_strip(p) : 0;
        p.tile_count = (const int*)(w + L.cell_off) + NCELL + 2;
        dim3 grid(dtype == 0 ? remap_grid(D, p.remap_mtiles) : remap_grid256(D, p.remap_mtiles), 1, 1);
        ProfRec rec = {nullptr, nullptr, (int)g_prof.size()};
        if (g_prof_on && !g_prof_rows) (void)hipMalloc(&g_prof_rows, PROF_MAX * sizeof(int));
        if (g_prof_on && g_prof_rows && rec.slot < PROF_MAX) {
            (void)hipMemcpyAsync(g_prof_rows + rec.slot, w + L.cell_off + NCELL * sizeof(int), sizeof(int),
                                 hipMemcpyDeviceToDevice, st);
            (void)hipEventCreate(&rec.a);
            (void)hipEventCreate(&rec.b);
            (void)hipEventRecord(rec.a, st);
        }
        if (dtype == 0) hipLaunchKernelGGL((gemm_kernel<float, false>), grid, dim3(GTHREADS), 0, st, p);
        else if (walk != 0) gemm_walk_launch(p, walk, 1, st);
        else if (use_gemm_phase(D)) hipLaunchKernelGGL((gemm_phase_kernel<EPI_STORE, false>), grid, dim3(G2_THREADS), 0, st, p);
        else hipLaunchKernelGGL((gemm_big_kernel<256, EPI_STORE, false>), grid, dim3(G2_THREADS), 0, st, p);
        if (g_prof_on && g_prof_rows && rec.slot < PROF_MAX) {
            (void)hipEventRecord(rec.b, st);
            g_prof.push_back(rec);
        }
    }
    {
        const long graphs = (num_nodes + nmax - 1) / nmax;
        const int npb = combine_npb_flag();
#define FPM_COMB(T_, N_)                                                                                         \
    do {                                                                                                         \
        const dim3 cg((unsigned)(((graphs + 7) / 8) * 8 * ((nmax + N_ - 1) / N_)));                              \
        const size_t lds = (size_t)combine_lds_kb_flag() * 1024;                                                 \
        if (combine_store_sc1_flag() && !(mode >> 1))                                                            \
            hipLaunchKernelGGL((combine_kernel<T_, N_, false, 16>), cg, dim3(64 * N_), lds, st, (const T_*)y_ws, \
                               (const int*)(w + L.cell_off), bias, (const int*)(w + L.dst_ptr),                 \
                               (const int4*)(w + L.rows4), (const float4*)(w + L.basis4), num_nodes, nmax,       \
                               nvalid, mode, xres, cscale, out_f, (T_*)out_t, nullptr);                          \
        else                                                                                                     \
            hipLaunchKernelGGL((combine_kernel<T_, N_>), cg, dim3(64 * N_), lds, st, (const T_*)y_ws,            \
                               (const int*)(w + L.cell_off), bias, (const int*)(w + L.dst_ptr),                 \
                               (const int4*)(w + L.rows4), (const float4*)(w + L.basis4), num_nodes, nmax,       \
                               nvalid, mode, xres, cscale, out_f, (T_*)out_t, nullptr);                          \
    } while (0)
        if (argmax) {
#define FPM_COMBA(T_)                                                                                            \
    hipLaunchKernelGGL((combine_kernel<T_, 4, true>), dim3((unsigned)(((graphs + 7) / 8) * 8 * ((nmax + 3) / 4))), \
                       dim3(256), 0, st, (const T_*)y_ws, (const int*)(w + L.cell_off), bias,                    \
                       (const int*)(w + L.dst_ptr), (const int4*)(w + L.rows4), (const float4*)(w + L.basis4),   \
                       num_nodes, nmax, nvalid, mode, xres, cscale, out_f, (T_*)out_t, argmax)
            if (dtype == 0) FPM_COMBA(float); else FPM_COMBA(bf16_t);
#undef FPM_COMBA
        } else if (dtype == 0) {
            if (npb == 16) FPM_COMB(float, 16); else if (npb == 8) FPM_COMB(float, 8); else FPM_COMB(float, 4);
        } else {
            if (npb == 16) FPM_COMB(bf16_t, 16); else if (npb == 8) FPM_COMB(bf16_t, 8); else FPM_COMB(bf16_t, 4);
        }
#undef FPM_COMB
    }
    return check_launch("fpm_spline_conv_fwd");
}

// Xe[e] = x[src] - x[dst]  (vertex_attr_to_edge_attr, spline_conv.py:73-81; feeds only the dead
// edge affinity Ke, computed on request).
namespace {
__global__ void edge_diff_kernel(const float* __restrict__ x, const int* __restrict__ src,
                                 const int* __restrict__ dst, long E, int D, float* __restrict__ out) {
    long e = blockIdx.x;
    if (e >= E) return;
    const float* a = x + (long)src[e] * D;
    const float* b = x + (long)dst[e] * D;
    for (int c = threadIdx.x; c < D; c += blockDim.x) out[e * D + c] = a[c] - b[c];
}

// Padded per-pair layout for the quadratic affinity GEMM: out[row[e]] = (x[src]-x[dst]) o c[pair[e]]
// (Xe * coefficients, affinity_layer.py:15); rows not named by any edge are left untouched.
__global__ void edge_diff_padded_kernel(const float* __restrict__ x, const int* __restrict__ src,
                                        const int* __restrict__ dst, const int* __restrict__ pair,
                                        const int* __restrict__ row, const float* __restrict__ cscale, long E, int D,
                                        float* __restrict__ out) {
    long e = blockIdx.x;
    if (e >= E) return;
    const float* a = x + (long)src[e] * D;
    const float* b = x + (long)dst[e] * D;
    const float* c = cscale ? cscale + (long)pair[e] * D : nullptr;
    float* o = out + (long)row[e] * D;
    for (int k = threadIdx.x; k < D; k += blockDim.x) {
        float v = a[k] - b[k];
        o[k] = c ? v * c[k] : v;
    }
}
}  // namespace

extern "C" int fpm_edge_diff_padded(const float* x, const int* src, const int* dst, const int* pair, const int* row,
                                    const float* cscale, long E, int D, float* out, void* stream) {
    if (E <= 0) return 0;
    FPM_CHECK_ARG(pair && row && D > 0, "edge_diff_padded: pair/row maps required");
    hipLaunchKernelGGL(edge_diff_padded_kernel, dim3((unsigned)E), dim3(256), 0, (hipStream_t)stream, x, src, dst,
                       pair, row, cscale, E, D, out);
    return fpm::check_launch("fpm_edge_diff_padded");
}

extern "C" int fpm_edge_diff(const float* x, const int* src, const int* dst, long E, int D, float* out, void* stream) {
    if (E <= 0) return 0;
    hipLaunchKernelGGL(edge_diff_kernel, dim3((unsigned)E), dim3(256), 0, (hipStream_t)stream, x, src, dst, E, D, out);
    return fpm::check_launch("fpm_edge_diff");
}

// Probe x gallery batches (C4): the shared side-0 graph's SplineConv output y (rows x 768, fp32) is
// computed once and broadcast to the B pairs, scaled per pair like the combine epilogue does
// (out_t[b] = T(y o c[b]), the X1 o c operand of the vertex affinity, affinity_layer.py:15), so
// results equal the per-pair path bit for bit.
namespace {
template <typename T>
__global__ void rows_bcast_scale_kernel(const float* __restrict__ y, long rows, int B, const float* __restrict__ coef,
                                        float* __restrict__ out_f, T* __restrict__ out_t, int split) {
    const long n = rows * 768;
    const int b = blockIdx.y;
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long)gridDim.x * blockDim.x) {
        const float v = y[k];
        if (out_f) out_f[(long)b * n + k] = v;
        if (!out_t) continue;
        const float z = coef ? v * coef[(long)b * 768 + (k % 768)] : v;
        if (split) {                       // the combine's split operand rows (mode >> 1)
            const T hi = fpm::from_f<T>(z), lo = fpm::from_f<T>(z - fpm::to_f<T>(hi));
            T* o = out_t + ((long)b * rows + k / 768) * 2304 + (k % 768);
            o[0] = hi;
            o[768] = split == 1 ? lo : hi;
            o[1536] = split == 1 ? hi : lo;
        } else {
            out_t[(long)b * n + k] = fpm::from_f<T>(z);
        }
    }
}
}  // namespace

extern "C" int fpm_rows_bcast_scale(int dtype, const float* y, long rows, int B, const float* coef, float* out_f,
                                    void* out_t, int split, void* stream) {
    FPM_CHECK_ARG(dtype == 0 || dtype == 1, "rows_bcast_scale: bad dtype");
    FPM_CHECK_ARG(split >= 0 && split <= 2 && (split == 0 || dtype == 1), "rows_bcast_scale: split needs bf16");
    if (B == 0 || rows == 0) return 0;
    dim3 grid((unsigned)((rows * 768 + 255) / 256 < 1024 ? (rows * 768 + 255) / 256 : 1024), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0)
        hipLaunchKernelGGL(rows_bcast_scale_kernel<float>, grid, dim3(256), 0, st, y, rows, B, coef, out_f, (float*)out_t,
                           0);
    else
        hipLaunchKernelGGL(rows_bcast_scale_kernel<bf16_t>, grid, dim3(256), 0, st, y, rows, B, coef, out_f,
                           (bf16_t*)out_t, split);
    return fpm::check_launch("fpm_rows_bcast_scale");
}

// Enrolled gallery (1:N identification): the cached fp32 SplineConv output rows of G graphs
// (concatenated, graph g at rows [row_off[g], row_off[g + 1])) gathered into the padded per-pair
// layout of a batch: pair b takes graph idx[b]; rows past its n_g are zeros.  The values are those of
// rows_bcast_scale_kernel (out_f = y, out_t = T(y o coef[b]), the same split patterns); the y * coef
// product is pinned (__fmul_rn) so that z - hi cannot be contracted into an FMA with it.
// An HBM-bound copy: a workgroup of 192 threads takes a band of GATHER_BAND rows of one pair, two rows
// per step, each thread 8 channels (two 16-B loads; 16-B stores, bf16 packed 8 per store).
namespace {
constexpr int GATHER_BAND = 16;

template <typename T> struct GatherStore;
template <> struct GatherStore<float> {
    static __device__ __forceinline__ void put(float* p, const float (&v)[8]) {
        *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
        *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
};
template <> struct GatherStore<bf16_t> {
    static __device__ __forceinline__ void put(bf16_t* p, const float (&v)[8]) {
        *(uint4*)p = make_uint4(fpm::f2bf2(v[0], v[1]), fpm::f2bf2(v[2], v[3]), fpm::f2bf2(v[4], v[5]),
                                fpm::f2bf2(v[6], v[7]));
    }
};

template <typename T, int SPLIT>
__global__ __launch_bounds__(192) void rows_gather_scale_kernel(const float* __restrict__ y,
                                                                const long* __restrict__ row_off,
                                                                const int* __restrict__ idx, int G, int nmax,
                                                                const float* __restrict__ coef,
                                                                float* __restrict__ out_f, T* __restrict__ out_t) {
    const int b = blockIdx.y;
    const int g = idx[b];
    if (g < 0 || g >= G) return;                       // the wrapper checks the range; never read outside y
    const long r0 = row_off[g];
    const long ng_l = row_off[g + 1] - r0;
    const int ng = ng_l < nmax ? (int)ng_l : nmax;
    const int sub = threadIdx.x >= 96 ? 1 : 0;         // which of the step's two rows
    const int c0 = 8 * (threadIdx.x - 96 * sub);       // this thread's 8 channels
    float cs[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
    if (coef && out_t) {
        const float4 a = *(const float4*)(coef + (long)b * 768 + c0), c = *(const float4*)(coef + (long)b * 768 + c0 + 4);
        cs[0] = a.x; cs[1] = a.y; cs[2] = a.z; cs[3] = a.w; cs[4] = c.x; cs[5] = c.y; cs[6] = c.z; cs[7] = c.w;
    }
    const int band0 = blockIdx.x * GATHER_BAND;
    constexpr int ldt = SPLIT ? 2304 : 768;
    for (int s = 0; s < GATHER_BAND; s += 2) {
        const int r = band0 + s + sub;
        if (r >= nmax) break;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (r < ng) {
            const float* src = y + (r0 + r) * 768 + c0;
            const float4 a = *(const float4*)src, c = *(const float4*)(src + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = c.x; v[5] = c.y; v[6] = c.z; v[7] = c.w;
        }
        const long row = (long)b * nmax + r;
        if (out_f) GatherStore<float>::put(out_f + row * 768 + c0, v);
        if (!out_t) continue;
        float z[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = (coef && r < ng) ? __fmul_rn(v[j], cs[j]) : v[j];   // padding: +0
        T* o = out_t + row * ldt + c0;
        if constexpr (SPLIT != 0) {
            float hi[8], lo[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                hi[j] = fpm::to_f<T>(fpm::from_f<T>(z[j]));
                lo[j] = z[j] - hi[j];
            }
            GatherStore<T>::put(o, hi);
            GatherStore<T>::put(o + 768, SPLIT == 1 ? lo : hi);
            GatherStore<T>::put(o + 1536, SPLIT == 1 ? hi : lo);
        } else {
            GatherStore<T>::put(o, z);
        }
    }
}
}  // namespace

extern "C" int fpm_rows_gather_scale(int dtype, const float* y, const long* row_off, const int* idx, int G, int B,
                                     int nmax, const float* coef, float* out_f, void* out_t, int split,
                                     void* stream) {
    FPM_CHECK_ARG(dtype == 0 || dtype == 1, "rows_gather_scale: bad dtype");
    FPM_CHECK_ARG(split >= 0 && split <= 2 && (split == 0 || dtype == 1), "rows_gather_scale: split needs bf16");
    FPM_CHECK_ARG(G > 0 && B >= 0 && nmax >= 0 && B <= 65535, "rows_gather_scale: bad sizes (G %d, B %d, nmax %d)", G,
                  B, nmax);
    FPM_CHECK_ARG(y && row_off && idx, "rows_gather_scale: y, row_off and idx are required");
    if (B == 0 || nmax == 0 || (!out_f && !out_t)) return 0;
    dim3 grid((unsigned)((nmax + GATHER_BAND - 1) / GATHER_BAND), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
#define FPM_GATHER(T_, S_)                                                                                     \
    hipLaunchKernelGGL((rows_gather_scale_kernel<T_, S_>), grid, dim3(192), 0, st, y, row_off, idx, G, nmax, coef, \
                       out_f, (T_*)out_t)
    if (dtype == 0) FPM_GATHER(float, 0);
    else if (split == 0) FPM_GATHER(bf16_t, 0);
    else if (split == 1) FPM_GATHER(bf16_t, 1);
    else FPM_GATHER(bf16_t, 2);
#undef FPM_GATHER
    return fpm::check_launch("fpm_rows_gather_scale");
}

extern "C" int fpm_profile_enable(int on) {
    g_prof_on = on != 0;
    return 0;
}

extern "C" int fpm_profile_enabled(void) { return g_prof_on ? 1 : 0; }

// Sum of the recorded edge-GEMM durations (ms) and algorithmic FLOPs since the last read.
extern "C" int fpm_profile_read(double* ms_total, double* flops_total, int* count) {
    double ms = 0.0, fl = 0.0;
    for (auto& r : g_prof) {
        float t = 0.f;
        if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) {
            fpm::set_error("fpm_profile_read: event query failed");
            return 2;
        }
        int rows = 0;
        if (hipMemcpy(&rows, g_prof_rows + r.slot, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) {
            fpm::set_error("fpm_profile_read: row count read failed");
            return 2;
        }
        ms += t;
        fl += 2.0 * rows * 768.0 * 768.0;
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    if (count) *count = (int)g_prof.size();
    g_prof.clear();
    if (ms_total) *ms_total = ms;
    if (flops_total) *flops_total = fl;
    return 0;
}

extern "C" int fpm_cast_bf16(const float* x, void* out, long n, void* stream);

// Product-row bookkeeping of a plan for the weight gradient: arows[r] = source node of product row
// r; cell_off[0..26] = row ranges per cell (cell 25 = the root weight).  Device pointers.
extern "C" int fpm_spline_plan_rows(void* ws, long E, long num_nodes, int** arows, int** cell_off) {
    PlanLayout L = plan_layout(E, num_nodes);
    *arows = (int*)((char*)ws + L.arows);
    *cell_off = (int*)((char*)ws + L.cell_off);
    return 0;
}

// Per-CSR-slot tables of a plan (E entries each): csr_e[p] = the edge in slot p, rows4[p] = its 4
// product rows (corner order s = 0..3), basis4[p] = its 4 basis weights.  Device pointers.
extern "C" int fpm_spline_plan_edges(void* ws, long E, long num_nodes, int** csr_e, int** rows4, float** basis4) {
    PlanLayout L = plan_layout(E, num_nodes);
    *csr_e = (int*)((char*)ws + L.csr_e);
    *rows4 = (int*)((char*)ws + L.rows4);
    *basis4 = (float*)((char*)ws + L.basis4);
    return 0;
}

// Backward of one SplineConv layer w.r.t. its input rows (the weight gradient is the caller's
// grouped X^T dY product over the same row ranges):
//   dY   = combine backward (max routing, root rows)                     fp32, max_rows x 768
//   dXr  = dY_cell W_cell^T per product row: the forward's grouped GEMM with the weights in the
//          reference's [cell][in][out] layout as the B operand (Wb, 26 x 768 x 768, operand dtype)
//   dX   = per-node sum of its rows' dXr (accumulate: dX += ...)
// y_ws: the forward's product rows of this layer; dY_op: bf16 copy of dY (dtype 1 only).
extern "C" int fpm_spline_conv_bwd_data_scatter(int dtype, const void* plan_ws, const void* rplan_ws,
                                                const int* argmax, long E, long num_nodes, int nmax,
                                                const int* nvalid, const void* Wb, const void* y_ws, int mode,
                                                const float* gout, const float* hout, float* dY, void* dY_op,
                                                float* dXrows, float* dX, int accumulate, void* stream);

extern "C" int fpm_spline_conv_bwd_data(int dtype, const void* plan_ws, long E, long num_nodes, int nmax,
                                        const int* nvalid, const void* Wb, const void* y_ws, int mode,
                                        const float* gout, const float* hout, float* dY, void* dY_op,
                                        float* dXrows, float* dX, int accumulate, void* stream) {
    return fpm_spline_conv_bwd_data_scatter(dtype, plan_ws, nullptr, nullptr, E, num_nodes, nmax, nvalid, Wb, y_ws,
                                            mode, gout, hout, dY, dY_op, dXrows, dX, accumulate, stream);
}

// fpm_set_tuning("scatter_f32_rows", 1) (env FPM_SCATTER_F32_ROWS): the bf16 scatter backward also
// writes the cell rows of the fp32 dY (off by default: only the root rows there)
int& scatter_f32_rows_flag() {
    static int v = [] {
        const char* e = getenv("FPM_SCATTER_F32_ROWS");
        return e ? atoi(e) : 0;
    }();
    return v;
}

// fpm_set_tuning("scatter_batch", 1 | 4) (env FPM_SCATTER_BATCH): out-edges per load batch of the
// scatter backward (same sums, same order)
int& scatter_batch_flag() {
    static int v = [] {
        const char* e = getenv("FPM_SCATTER_BATCH");
        return e ? atoi(e) : 4;
    }();
    return v;
}

// rplan_ws (the plan of the reversed edges: its CSR lists each node's out-edges) + argmax (from
// fpm_spline_conv_fwd_argmax): the atomic-free scatter backward; both null: the atomic one.
extern "C" int fpm_spline_conv_bwd_data_scatter(int dtype, const void* plan_ws, const void* rplan_ws,
                                                const int* argmax, long E, long num_nodes, int nmax,
                                                const int* nvalid, const void* Wb, const void* y_ws, int mode,
                                                const float* gout, const float* hout, float* dY, void* dY_op,
                                                float* dXrows, float* dX, int accumulate, void* stream) {
    using namespace fpm;
    FPM_CHECK_ARG(dtype == 0 || dtype == 1, "spline_conv_bwd: bad dtype");
    FPM_CHECK_ARG(mode == 1 || (mode == 0 && hout), "spline_conv_bwd: mode 0 needs the layer output");
    FPM_CHECK_ARG(dtype == 0 || dY_op, "spline_conv_bwd: bf16 needs the dY operand buffer");
    FPM_CHECK_ARG((rplan_ws == nullptr) == (argmax == nullptr), "spline_conv_bwd: rplan and argmax go together");
    PlanLayout L = plan_layout(E, num_nodes);
    const char* w = (const char*)plan_ws;
    hipStream_t st = (hipStream_t)stream;
    const int D = 768;
    const unsigned nb = (unsigned)((num_nodes + 3) / 4);
    if (argmax) {
        // slot_of in the dXrows buffer (consumed before the GEMM overwrites it)
        FPM_CHECK_ARG(L.max_rows * D >= E, "spline_conv_bwd: scratch too small");
        int* slot_of = (int*)dXrows;
        const char* rw = (const char*)rplan_ws;
        hipLaunchKernelGGL(slot_of_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st,
                           (const int*)(w + L.csr_e), E, slot_of);
        const size_t lds = (size_t)(NCELL - 1) * D * sizeof(float);
        // every call (the attribute is per device; the call is cheap), like the forward kernels
        const int qb = scatter_batch_flag();
        FPM_CHECK_ARG(qb == 1 || qb == 4, "spline_conv_bwd: scatter_batch must be 1 or 4");
        auto kern = qb == 4 ? combine_scatter_bwd_kernel<4> : combine_scatter_bwd_kernel<1>;
        const hipError_t ae = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        FPM_CHECK_ARG(ae == hipSuccess, "spline_conv_bwd: %zu B of LDS refused: %s", lds, hipGetErrorString(ae));
        hipLaunchKernelGGL(kern, dim3((unsigned)num_nodes), dim3(D), lds, st,
                           (const int*)(w + L.cell_off), (const int*)(w + L.rowid), (const int*)(w + L.mask),
                           (const int*)(w + L.grp_e), (const float*)(w + L.basis_e), (const int*)(rw + L.dst_ptr),
                           (const int*)(rw + L.csr_e), (const int*)(rw + L.nbr_local), (const int*)slot_of, argmax,
                           num_nodes, nmax, nvalid, mode, gout, hout, dY, dtype == 1 ? (bf16_t*)dY_op : nullptr,
                           (dtype == 0 || scatter_f32_rows_flag()) ? 1 : 0);
    } else {
    (void)hipMemsetAsync(dY, 0, (size_t)L.max_rows * D * sizeof(float), st);
    if (dtype == 0)
        hipLaunchKernelGGL((combine_bwd_kernel<float>), dim3(nb), dim3(256), 0, st, (const float*)y_ws,
                           (const int*)(w + L.cell_off), (const int*)(w + L.dst_ptr), (const int4*)(w + L.rows4),
                           (const float4*)(w + L.basis4), num_nodes, nmax, nvalid, mode, gout, hout, dY);
    else
        hipLaunchKernelGGL((combine_bwd_kernel<bf16_t>), dim3(nb), dim3(256), 0, st, (const bf16_t*)y_ws,
                           (const int*)(w + L.cell_off), (const int*)(w + L.dst_ptr), (const int4*)(w + L.rows4),
                           (const float4*)(w + L.basis4), num_nodes, nmax, nvalid, mode, gout, hout, dY);
    }
    if (dtype == 1 && !argmax) {
        int rc = fpm_cast_bf16(dY, dY_op, L.max_rows * D, stream);
        if (rc) return rc;
    }
    GemmParams p = {};
    p.A = dtype == 0 ? (const void*)dY : (const void*)dY_op; p.lda = D; p.a_rows = nullptr;
    p.B = Wb; p.ldb = D; p.sB_seg = (long)D * D;
    p.M = (int)L.max_rows; p.N = D; p.K = D; p.nseg = 1;
    p.group_off = (const int*)(w + L.cell_off);
    p.epi = EPI_STORE; p.ldc = D; p.Cf = dXrows;
    if (dtype == 0) {
        p.tile_info = (const int*)(w + L.tile_info);
        p.remap_mtiles = (int)L.max_tiles;
        hipLaunchKernelGGL((gemm_kernel<float, false>), dim3(remap_grid(D, p.remap_mtiles)), dim3(GTHREADS), 0, st, p);
    } else {
        p.tile_info = (const int*)(w + L.tile_info2);
        p.remap_mtiles = (int)L.max_tiles2;
        dim3 grid(remap_grid256(D, p.remap_mtiles));
        if (use_gemm_phase(D)) hipLaunchKernelGGL((gemm_phase_kernel<EPI_STORE, true>), grid, dim3(G2_THREADS), 0, st, p);
        else hipLaunchKernelGGL((gemm_big_kernel<256, EPI_STORE, true>), grid, dim3(G2_THREADS), 0, st, p);
    }
    hipLaunchKernelGGL(node_rows_sum_kernel, dim3(nb), dim3(256), 0, st, dXrows, (const int*)(w + L.rowid), num_nodes,
                       accumulate, dX);
    return check_launch("fpm_spline_conv_bwd_data");
}

// ---------------------------------------------------------------------------------------------
// SplineConv weight operands for a training step (the layer's weights change every step):
// the K cell matrices weight[k] (Cin x Cout, reference layout) and root (Cin x Cout) as K + 1 stacked
// matrices, optionally transposed to (Cout x Cin) -- the forward GEMM's B -- and optionally in bf16.
// One pass per copy (64 x 64 tiles through LDS for the transposed form) instead of the transpose /
// concatenate / cast sequence of separate torch kernels.
namespace {

template <typename TO, bool TRANS>
__global__ __launch_bounds__(256) void spline_w_pack_kernel(const float* __restrict__ weight,
                                                            const float* __restrict__ root, int K, int Cin, int Cout,
                                                            TO* __restrict__ out) {
    __shared__ float t[64][65];
    const int k = blockIdx.z;
    const float* src = k < K ? weight + (long)k * Cin * Cout : root;
    TO* dst = out + (long)k * Cin * Cout;
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;   // tile of the source (rows = Cin)
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    if (!TRANS) {
        for (int r = ty; r < 64; r += 4) {
            const int rr = r0 + r, cc = c0 + tx;
            if (rr < Cin && cc < Cout) dst[(long)rr * Cout + cc] = fpm::from_f<TO>(src[(long)rr * Cout + cc]);
        }
        return;
    }
    for (int r = ty; r < 64; r += 4) {
        const int rr = r0 + r, cc = c0 + tx;
        t[r][tx] = (rr < Cin && cc < Cout) ? src[(long)rr * Cout + cc] : 0.f;
    }
    __syncthreads();
    for (int c = ty; c < 64; c += 4) {
        const int cc = c0 + c, rr = r0 + tx;
        if (cc < Cout && rr < Cin) dst[(long)cc * Cin + rr] = fpm::from_f<TO>(t[tx][c]);
    }
}

}  // namespace

// out: (K + 1) stacked matrices, [k][Cout][Cin] (transpose = 1) or [k][Cin][Cout] (0); dtype 0 fp32,
// 1 bf16
extern "C" int fpm_spline_weight_pack(const float* weight, const float* root, int K, int Cin, int Cout, int transpose,
                                      int dtype, void* out, void* stream) {
    FPM_CHECK_ARG(K >= 0 && Cin > 0 && Cout > 0 && weight && root && out, "spline_weight_pack: bad arguments");
    FPM_CHECK_ARG(dtype == 0 || dtype == 1, "spline_weight_pack: bad dtype");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((Cout + 63) / 64), (unsigned)((Cin + 63) / 64), (unsigned)(K + 1));
    if (dtype == 1) {
        if (transpose) hipLaunchKernelGGL((spline_w_pack_kernel<bf16_t, true>), grid, dim3(256), 0, st, weight, root, K, Cin, Cout, (bf16_t*)out);
        else hipLaunchKernelGGL((spline_w_pack_kernel<bf16_t, false>), grid, dim3(256), 0, st, weight, root, K, Cin, Cout, (bf16_t*)out);
    } else {
        if (transpose) hipLaunchKernelGGL((spline_w_pack_kernel<float, true>), grid, dim3(256), 0, st, weight, root, K, Cin, Cout, (float*)out);
        else hipLaunchKernelGGL((spline_w_pack_kernel<float, false>), grid, dim3(256), 0, st, weight, root, K, Cin, Cout, (float*)out);
    }
    return fpm::check_launch("fpm_spline_weight_pack");
}

"""The strip-walk product GEMM (gemm_walk_kernel, gemm_phase.h): strips of two row tiles per workgroup
with the LDS-DMA stream carried across the tile boundary.  Every case compares bit for bit (torch.equal)
against the two-stage kernel gemm_big_kernel<256> (tuning gemm_phase = 0), whose per-element
accumulation order the walk keeps."""
import pytest
import torch

import fpm
from fpm import ops, params, synth
from fpm.batch import DeviceBatch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = 3.0
PAD_ROWS = 300          # output rows past M, pre-filled with the sentinel
AUTO = 8                # gemm_walk: the strip length is the kernel's choice (the default)


class _tuning:
    """Set tuning keys for a block, restore them after it."""

    def __init__(self, **kv):
        self.kv, self.prev = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.prev[k] = ops.set_tuning(k, v)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            ops.set_tuning(k, v)


def _gemm(A, Bm, rows, M, N, K, batch, bias=None):
    """Gathered-row batched bf16 GEMM into a sentinel-filled output with PAD_ROWS spare rows."""
    out = torch.full((batch, M + PAD_ROWS, N), SENTINEL, device=DEV, dtype=torch.bfloat16)
    ops.gemm(A, Bm, M, N, K, K, K, batch=batch, sA=A.shape[1] * K, sB=N * K, sC=(M + PAD_ROWS) * N, a_rows=rows,
             bias=bias, out_t=out)
    torch.cuda.synchronize()
    return out


# M per strip length S: 256 S + 1 (a one-row strip tail), 256 S - 1 (a partial last tile), and 700
# (fewer tiles than one strip of 3 or 4; a partial last tile for 2)
M_CASES = sorted({256 * s + d for s in (1, 2, 3, 4) for d in (1, -1)} | {700})


@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("K", [128, 192, 768])   # 2 K-tiles (prologue runs into the carry-over), odd count, the product shape
def test_gemm_walk_bit_identical(K, N):
    """ops.gemm with gathered rows: gemm_walk 1 (the phase kernel), 2, 3, 4 (every forced value is a
    strip of two: the kernel has no longer ones) and the default rule, each with plain and with sc1
    stores (gemm_walk_kernel<false> / <true>; fpm_gemm passes gemm_store_sc1 on), equal the two-stage
    kernel; the rows past M keep their sentinel.  The batch count brings these small M over
    fpm_gemm's thresholds for the 256-row kernels."""
    g = torch.Generator().manual_seed(K * 7 + N)
    batch = 32 if N == 256 else 11
    src_rows = max(M_CASES) + 17
    A = (torch.randn(batch, src_rows, K, generator=g) * 0.1).to(torch.bfloat16).to(DEV)
    Bm = (torch.randn(batch, N, K, generator=g) * 0.1).to(torch.bfloat16).to(DEV)
    for M in M_CASES:
        rows = torch.randint(0, src_rows, (M,), generator=g).int().to(DEV)
        with _tuning(gemm_bn256_min=1, gemm_phase=0):
            ref = _gemm(A, Bm, rows, M, N, K, batch)
        assert torch.all(ref[:, M:] == SENTINEL)
        assert not torch.all(ref[:, :M] == SENTINEL)
        for walk in (1, 2, 3, 4, AUTO):
            for sc1 in (0, 1):
                with _tuning(gemm_bn256_min=1, gemm_walk=walk, gemm_store_sc1=sc1):
                    out = _gemm(A, Bm, rows, M, N, K, batch)
                assert torch.equal(out, ref), (M, walk, sc1)


def test_gemm_walk_bias_bit_identical():
    """The bias branch of the walk's epilogue (4 consecutive columns per lane)."""
    g = torch.Generator().manual_seed(5)
    M, N, K, batch = 769, 512, 192, 16
    A = (torch.randn(batch, M + 17, K, generator=g) * 0.1).to(torch.bfloat16).to(DEV)
    Bm = (torch.randn(batch, N, K, generator=g) * 0.1).to(torch.bfloat16).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    rows = torch.randint(0, M + 17, (M,), generator=g).int().to(DEV)
    with _tuning(gemm_bn256_min=1, gemm_phase=0):
        ref = _gemm(A, Bm, rows, M, N, K, batch, bias=bias)
    for walk in (2, 3):
        with _tuning(gemm_bn256_min=1, gemm_walk=walk):
            assert torch.equal(_gemm(A, Bm, rows, M, N, K, batch, bias=bias), ref), walk


@pytest.mark.parametrize("M", [0, 5, 256])
def test_gemm_walk_tiny_launches(M):
    """With the walk forced on: a single full tile per batch entry (M = 256: a strip of one tile
    on the walk kernel).  M = 0 and M = 5 never reach it -- fpm_gemm returns at once for no rows and
    takes its small tile below 256 rows; they only pin that forcing the walk changes neither."""
    g = torch.Generator().manual_seed(M)
    N, K, batch = 256, 128, 140
    A = (torch.randn(batch, 8, K, generator=g) * 0.1).to(torch.bfloat16).to(DEV)
    Bm = (torch.randn(batch, N, K, generator=g) * 0.1).to(torch.bfloat16).to(DEV)
    rows = torch.randint(0, 8, (max(M, 1),), generator=g).int().to(DEV)
    with _tuning(gemm_bn256_min=1, gemm_phase=0):
        ref = _gemm(A, Bm, rows, M, N, K, batch)
    with _tuning(gemm_bn256_min=1, gemm_walk=3):
        out = _gemm(A, Bm, rows, M, N, K, batch)
    assert torch.equal(out, ref)
    assert torch.all(out[:, M:] == SENTINEL)


@pytest.fixture(scope="module")
def sd():
    return params.init_params(7)


def test_gemm_walk_grouped_spline(sd):
    """The grouped SplineConv product GEMM on 20 graphs of 40 keypoints: the 26 cell groups hold a
    few rows to a few hundred rows each, so strips straddle group boundaries, most groups end in a
    partial tile, and with an odd tile count the last strip has one tile.  Product rows and layer
    output of gemm_walk 2, 3, 4 and the rule, with plain and with sc1 stores, against gemm_walk 0
    (the phase kernel); the workspace past the last product row keeps its fill.  (The plan pads its
    tile table only after the last real tile and the kernel stops at the plan's tile count, so a
    padded entry inside a strip does not occur on this path.)"""
    pairs = synth.make_batch(31, 20, 40)
    bt = DeviceBatch.from_pairs(pairs, DEV)
    net = fpm.Net(regression=True, backbone=False, dtype="bf16")
    net.load_state_dict(sd)
    wp = net.packed(DEV)
    side, nm = 0, bt.nmax[0]
    nn_, E = bt.B * nm, bt.E[side]
    plan = ops.spline_plan(bt.src[side], bt.dst[side], bt.pseudo[side], nn_, nm, bt.max_graph_edges(side))
    _, cell_off = ops.spline_plan_rows(plan, E, nn_)
    prod_rows = int(cell_off[26].item())
    assert prod_rows > 26 * 8
    assert any(int(cell_off[c + 1] - cell_off[c]) % 256 for c in range(26))      # partial last tiles
    x_op = ops.cast_bf16(bt.x[side])
    used = prod_rows * 768 * 2

    def run(walk, sc1):
        yws = ops.spline_y_ws(ops.BF16, E, nn_, DEV)
        yws.fill_(0x5a)
        h = torch.empty(nn_, 768, device=DEV, dtype=torch.bfloat16)
        with _tuning(gemm_walk=walk, gemm_store_sc1=sc1):
            ops.spline_conv(x_op, plan, E, nn_, nm, bt.n[side], wp["W0"], wp["bias0"], yws, 0, out_t=h)
            torch.cuda.synchronize()
        return yws, h

    ref_y, ref_h = run(0, 0)
    assert torch.all(ref_y[used:] == 0x5a)
    for walk in (2, 3, 4, AUTO):
        for sc1 in (0, 1):
            yws, h = run(walk, sc1)
            assert torch.equal(yws[:used], ref_y[:used]), (walk, sc1)
            assert torch.all(yws[used:] == 0x5a), (walk, sc1)   # nothing written past the last product row
            assert torch.equal(h, ref_h), (walk, sc1)


def test_gemm_walk_forward_bit_identical(sd):
    """The whole bf16 forward at n = 96 (as test_gnn_kernel_variants_bit_identical): gemm_walk 0, 3
    (strips of two forced) and the default rule give the same outputs bit for bit."""
    pairs = synth.make_batch(17, 3, 96)
    net = fpm.Net(regression=True, backbone=False, dtype="bf16")
    net.load_state_dict(sd)
    bt = DeviceBatch.from_pairs(pairs, DEV)
    outs = []
    for walk in (0, 3, AUTO):
        with _tuning(gemm_walk=walk):
            r = net.run(bt, chunks=1)
            torch.cuda.synchronize()
        outs.append(r)
    for r in outs[1:]:
        for k in ("s", "ss", "ds_mat", "k_prob"):
            assert torch.equal(r[k], outs[0][k]), k

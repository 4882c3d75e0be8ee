"""CPU checks of tests/gnn_ref.py, the float64 reference and the gates that tests/test_gnn_stages.py
holds the GNN layer and readout kernels to.  Nothing here needs a GPU.

  pattern      the materialised Kronecker pattern and its factorisation agree to 1e-14 on every box of
               up to 65 keypoints (and on a 260 x 24 box), C = 1 and 17: the two aggregation forms the
               reference uses are one function.
  not tight    the fp32 CPU evaluation of the reference formula sits inside every gate of the stage
               tests on every case (largest fraction of a gate here: 0.08 for x1, 0.012 for z,
               0.16 for z from its own x1).
  not loose    each deliberate mistake, applied to the reference, leaves the gate by the factor below
               at its worst element (the largest over the boxes up to 65 keypoints; the smallest over
               those boxes in brackets).  A kernel with that mistake therefore fails the GPU
               comparison: its distance from the reference is the mistake's, less a gate at most.
                                                                        C = 1              C = 17
                 diag_block     diagonal masked by the valid block      2.7e5 (9.5e4)      1.2e5 (8.5e4)
                 swap_edges     in- and out-edges of graph 1 swapped    4.3e5 (1.3e5)      8.1e4 (7.1e4)
                 drop_tail      last neighbour of a list >= 5 dropped   9.7e4 (2.9e4)      2.3e4 (1.3e4)
                 count_no_diag  count without the +1 of the diagonal    3.1e5 (9.6e4)      7.6e4 (5.1e4)
                 lin_r_on_agg   lin_r applied to agg                    5.7e5 (1.6e5)      1.6e5 (1.1e5)
                 swap_ch_15_16  input channels 15 and 16 swapped        -                  1.8e5 (9.6e4)
  chain        the oracle's fp32-vs-float64 distance of the chained case (three layers with their
               Sinkhorns, then the readout; init_params(7), Kp = rand on the valid block) per pair:
               the figure gate D of the stage tests is 8 x of.
"""
import functools

import pytest
import torch

import gnn_ref as R

SMALL = [s for s, v in R.STAGE_SHAPES.items() if max(v[0], v[1]) <= R.EXPLICIT_MAX]
CHAIN = ["40x24", "24x40", "65x24", "257x24"]


def _pairs(shape):
    n1max, n2max, n1s, n2s = R.ALL_SHAPES[shape]
    _, l1, l2 = R._graphs(shape)
    for b, (n1b, n2b) in enumerate(zip(n1s, n2s)):
        yield b, n1b, n2b, l1[b], l2[b]


@pytest.mark.parametrize("shape", sorted(R.STAGE_SHAPES))
def test_stage_fixture_has_every_list_length(shape):
    """The boxes the stage tests add hold what the resident test's boxes hold: graph-2 lists of every
    length 0..7, a graph-1 node of degree 0 and one of degree 12, empty padded nodes."""
    n1max, n2max, n1s, n2s = R.ALL_SHAPES[shape]
    for b, n1b, n2b, l1, l2 in _pairs(shape):
        assert len(l1) == n1max and len(l2) == n2max
        assert {len(r) for r in l2[:n2b]} == set(range(8))
        d1 = [len(r) for r in l1[:n1b]]
        assert 0 in d1 and 12 in d1
        assert all(len(r) == 0 for r in l2[n2b:]) and all(len(r) == 0 for r in l1[n1b:])
    if shape == "16x12x9":
        assert len(n1s) == 9
    if shape == "24x40":
        assert n1max < n2max


def test_lists_are_in_edges():
    """l[i] holds the sources of the edges INTO i, and the fixture's graphs are not symmetric (a
    symmetric one cannot tell in-edges from out-edges)."""
    e = R.edge_index([[], [0, 2], [1]])
    assert e.tolist() == [[0, 2, 1], [1, 1, 2]]
    for shape in SMALL:
        for b, n1b, n2b, l1, l2 in _pairs(shape):
            for ll in (l1, l2):
                e = R.edge_index(ll)
                fwd = set(zip(e[0].tolist(), e[1].tolist()))
                assert any((d, s) not in fwd for s, d in fwd)


@pytest.mark.parametrize("C", [1, 17])
@pytest.mark.parametrize("shape", SMALL + ["260x24"])
def test_pattern_forms_agree(shape, C):
    """Explicit and factorised aggregation agree to 1e-14 (measured: at most 4.4e-16)."""
    n1max, n2max, _, _ = R.ALL_SHAPES[shape]
    g = torch.Generator().manual_seed(5 + C)
    worst = 0.0
    for b, n1b, n2b, l1, l2 in _pairs(shape):
        x = torch.randn(n1max * n2max, C, generator=g, dtype=torch.float64)
        e1, e2 = R.edge_index(l1), R.edge_index(l2)
        a = R.aggregate(x, e1, e2, n1max, n2max, n1b, n2b, explicit=True)
        f = R.aggregate(x, e1, e2, n1max, n2max, n1b, n2b, explicit=False)
        worst = max(worst, float((a - f).abs().max()))
    print("MEASURE pattern.%s.C%d err=%.3g" % (shape, C, worst))
    assert worst <= 1e-14


def test_unpack_follows_the_oracle_layer():
    """unpack(pack_layer(sd, l)) in ref_layer is oracle.gnn_layer's x1 on the same state dict."""
    import oracle as O
    sd = R.init_sd()
    n1max, n2max, n1s, n2s = R.ALL_SHAPES["24x40"]
    for C, l in ((1, 0), (17, 1)):
        X, W, _ = R.layer_case("24x40", C, "init")
        for b, n1b, n2b, l1, l2 in _pairs("24x40"):
            e1, e2 = R.edge_index(l1), R.edge_index(l2)
            x = R.pair_x(X, b).double()
            agg_fn = lambda v: O.pattern_mean_factorized(v, e1, e2, n1max, n2max, n1b, n2b)
            want = O.gnn_layer(x, sd, l, agg_fn, n1max, n2max, n1b, n2b)[:, :16]
            x1, _, _, _ = R.layer_reference("24x40", C, "init")[b]
            assert float((x1 - want).abs().max()) <= 1e-13


def _cases():
    return [(s, C, "rand") for s in R.STAGE_SHAPES for C in (1, 17)] + [("40x24", 1, "init"), ("40x24", 17, "init")]


@pytest.mark.parametrize("shape,C,kind", _cases())
def test_gates_hold_the_fp32_reference(shape, C, kind):
    """Gate not too tight: the same formula evaluated in fp32 on the CPU stays inside gate A (x1 and
    z against the full reference) and inside the z-from-own-x1 gate."""
    n1max, n2max, _, _ = R.ALL_SHAPES[shape]
    X, W, cls_w = R.layer_case(shape, C, kind)
    wc, bc = R.unpack(W, C)["wc"].double(), R.unpack(W, C)["bc"].double()
    for b, n1b, n2b, l1, l2 in _pairs(shape):
        x1, z, S, K = R.layer_reference(shape, C, kind)[b]
        x1f, zf, _ = R.ref_layer(R.pair_x(X, b), R.edge_index(l1), R.edge_index(l2), n1max, n2max, n1b, n2b, W, C,
                                 dtype=torch.float32)
        assert x1f.dtype == torch.float32
        f1 = float(((x1f.double() - x1).abs() / (K[:, None] * R.U * S["x1"])).max())
        fz = float(((zf.double() - z).abs() / ((K + 17) * R.U * S["z"])).max())
        own = x1f.double() @ wc + bc
        fo = float(((zf.double() - own).abs() / (17 * R.U * (x1f.double().abs() @ wc.abs() + bc.abs()))).max())
        print("MEASURE tight.%s.C%d.%s.b%d x1=%.3g z=%.3g z_own=%.3g" % (shape, C, kind, b, f1, fz, fo))
        assert f1 <= 1.0 and fz <= 1.0 and fo <= 1.0


@functools.lru_cache(maxsize=None)
def _mistake_factor(shape, C, mistake):
    """max over pairs and elements of |x1_mistaken - x1| / gate A."""
    n1max, n2max, _, _ = R.ALL_SHAPES[shape]
    X, W, _ = R.layer_case(shape, C, "rand")
    worst = 0.0
    for b, n1b, n2b, l1, l2 in _pairs(shape):
        x1, _, S, K = R.layer_reference(shape, C, "rand")[b]
        if mistake == "drop_tail":
            e1, e2, m = R.edge_index(R.drop_last_of_long(l1)), R.edge_index(R.drop_last_of_long(l2)), None
        else:
            e1, e2, m = R.edge_index(l1), R.edge_index(l2), mistake
        bad, _, _ = R.ref_layer(R.pair_x(X, b), e1, e2, n1max, n2max, n1b, n2b, W, C, explicit=True, mistake=m)
        worst = max(worst, float(((bad - x1).abs() / (K[:, None] * R.U * S["x1"])).max()))
    return worst


@pytest.mark.parametrize("mistake,C", [(m, C) for m in R.MISTAKES for C in (1, 17) if (m, C) != ("swap_ch_15_16", 1)])
def test_gates_reject_each_mistake(mistake, C):
    """Gate not too loose: the mistaken reference is at least 10 gates from the right one at some
    element of some box -- in fact on every box of up to 65 keypoints."""
    f = [_mistake_factor(s, C, mistake) for s in SMALL]
    print("MEASURE loose.%s.C%d max=%.3g min=%.3g" % (mistake, C, max(f), min(f)))
    assert max(f) >= 10.0
    assert min(f) >= 10.0


@pytest.mark.parametrize("shape", CHAIN)
def test_chain_conditioning(shape):
    """The fp32 oracle chain against the float64 one per pair.  Measured: layers 4e-7 to 2.2e-6, s
    1.2e-7 to 3.6e-7 at max|s| 0.2 to 0.4.  Held here: err32 of s is no less than the fp32 resolution
    of s (so that 8 x err32 is a gate a correct fp32 chain can meet without a floor) and no more than
    1e-5 (so that the gate stays under the 1e-4 the whole forward is held to elsewhere)."""
    X0, sd = R.chain_inputs(shape, 7), R.init_sd()
    l64, s64 = R.oracle_chain(shape, X0, sd, torch.float64)
    l32, s32 = R.oracle_chain(shape, X0, sd, torch.float32)
    for b in range(X0.shape[0]):
        el = [float((l32[l][b].double() - l64[l][b]).abs().max()) for l in range(3)]
        es, ms = float((s32[b].double() - s64[b]).abs().max()), float(s64[b].abs().max())
        print("MEASURE chain.%s.b%d layers=%.3g/%.3g/%.3g s=%.3g max|s|=%.3g" % ((shape, b) + tuple(el) + (es, ms)))
        assert R.U * ms <= es <= 1e-5
        assert max(el) <= 1e-4

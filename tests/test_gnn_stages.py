"""The association-graph GNN layer and the readout (csrc/gnn.hip; DESIGN rows a6, a7, a9) against the
float64 references of tests/gnn_ref.py: every kernel form of the layer, the schedule (ord2) and batch
composition, the readout with and without vpart, the three layers chained as Net issues them, and
the refusals.  The inputs are the hand-built directed graphs of gnn_ref._graphs (graph-2 lists of every
length 0..7, a graph-1 node of degree 0 and one of degree 12, pairs shorter than the box, empty
padded nodes) with random X over the whole box; tests/test_gnn_ref_cpu.py shows that the gates below
hold the fp32 CPU evaluation of the reference and reject six deliberate mistakes (a diagonal masked
by the valid block, swapped in- and out-edges, a dropped tail neighbour, a count without the
diagonal's +1, lin_r on agg, two swapped input channels) by >= 1e4 gates each.

Gates (u = 2^-24; nothing in them is measured on the GPU; S = the reference formula with |W|, |b|,
|x|, elementwise, from gnn_ref.ref_layer / ref_readout):
  A  x1: |dev - ref| <= K(p) u S(p) elementwise.  K(p) counts the fp32 roundings on the longest path
     to x1[p][o]: deg2(d) + deg1(i) + 1 adds of the two-level neighbour sum and the diagonal term, 2
     for the reciprocal and its multiply, C fmas of lin_l (lin_r and W1 are chains of the same length
     beside it, not behind it), 16 fmas of W2 (with its bias add: the MLP path is C + 17 long, shorter
     than the lin_l path whenever deg1 + deg2 >= 12, and the constant below covers both), and the 3
     adds of ((l + bl) + r) + u:   K(p) = deg1(i) + deg2(d) + C + 22.
     Each rounding is relative to a partial sum bounded by S(p); second-order terms (K u)^2 S are
     below 1e-5 of the gate.
     z and vpart from the device's own x1: 16 fmas (vpart) plus the bias add (z):
     |z - (wc . x1_dev + bc)| <= 17 u (|wc| . |x1_dev| + |bc|), float64 on the device's x1.
     z and vpart against the full reference: the x1 gate through the dot product plus the above,
     (K(p) + 17) u S_z(p) and (K(p) + 16) u S_vpart(p).
  C  readout: 3 u S with vpart (one fma, one add, one to spare), 19 u S without (17 multiply-adds,
     the bias add, one to spare).
  D  stage-isolated: layer l + 1's reference is fed the device's own layer-l output widened to
     float64, so gate A applies unchanged (and gate C to the readout).  End to end: |s - s64| <=
     8 x err32 per pair, err32 = the fp32 CPU oracle chain against the float64 one on the same
     inputs (1.2e-7 to 3.0e-7 here, test_gnn_ref_cpu.test_chain_conditioning; no floor).

Which case reaches which code (n = n1max; "resident" = gnn_layer_resident_kernel<C, 8>, "form 0" =
gnn_layer_kernel<C, SPOL, true, NSW>):
  route      tuning              n <= 256 (40x24 40x40 64x24 64x40 16x12x9 24x40 65x24 256x24)   n > 256 (257x24 600x16 1024x16)
  default    -                   resident<1, 8>, resident<17, 8>                                 form 0 <1>, <17>
  form0      gnn_form = 0        form 0 <1>, <17>                                                -
  sweeps2    gnn_sweeps = 2      form 0 <17, 0, true, 2> (C = 17)                                the same
  sweeps3    gnn_sweeps = 3      form 0 <17, 0, true, 3> (C = 17)                                the same
  sc1        gnn_store_sc1 = 1   form 0 <1, 16>, <17, 16>                                        the same
  every route in the plain form (Xout + z) and the last form (vpart + z, Xout not written).
  Threads per block: 64 (16x12x9, 24x40, 40x*, 64x*), 128 (65x24), 256, 320 (257x24), 640, 1024.
  1024x16 at C = 17 is the one launch with more than 64 KiB of dynamic LDS (80 KiB).
  24x40: n1max < n2max.  16x12x9: nine pairs, pair 8 in the second round of pair_block with seven
  padded pairs beside it.
  readout    node_classifier_t_kernel, vpart branch and 17-term branch, at (64, 64) one full tile,
             (65, 63) a one-row second tile along i, (13, 130) three tiles along d, (130, 13) three along i.

MEASURED: the largest fraction of its gate each check used (err / gate) over all cases of one run on
an MI355X.  The gates do not use these numbers.
"""
import functools

import pytest
import torch

import fpm
from fpm import _lib, config, ops
import gnn_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENT = 5.0
U = R.U

MEASURED = {
    # A, largest over boxes, C, plain / last and both weight sets.  The routes are bit-identical where
    # they share a box (test_gnn_resident_gpu.py and the sweeps / sc1 tests say so too); their figures
    # differ only by the boxes each one runs on
    "A.default.x1": 0.081, "A.default.z": 0.016, "A.default.z_own": 0.247, "A.default.vpart": 0.025,
    "A.form0.x1": 0.062, "A.form0.z": 0.016, "A.form0.z_own": 0.247, "A.form0.vpart": 0.017,
    "A.sweeps2.x1": 0.031, "A.sweeps2.z": 0.0066, "A.sweeps2.z_own": 0.247, "A.sweeps2.vpart": 0.0064,
    "A.sweeps3.x1": 0.031, "A.sweeps3.z": 0.0066, "A.sweeps3.z_own": 0.247, "A.sweeps3.vpart": 0.0064,
    "A.sc1.x1": 0.081, "A.sc1.z": 0.016, "A.sc1.z_own": 0.247, "A.sc1.vpart": 0.025,
    # 1024x16 alone (C = 17 is the 80 KiB launch): x1 0.079 (C = 1) / 0.026 (C = 17), z_own 0.204
    "A.1024x16.x1": 0.079, "A.1024x16.z_own": 0.204,
    "C.full": 0.193, "C.vpart": 0.597,
    "D.layer.x1": 0.048, "D.layer.z": 0.010, "D.layer.vpart": 0.0035, "D.readout": 0.524,
    # end to end: |s - s64| 1.2e-7 to 4.4e-7 against gates of 9.6e-7 to 3.1e-6
    "D.s": 0.291,
}

BOXES = [s for s in R.STAGE_SHAPES if s != "1024x16"]
CHAIN = ["40x24", "24x40", "65x24", "257x24"]


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


def _gate(tag, dev, ref, gate):
    """|dev - ref| <= gate elementwise; prints the worst fraction before asserting."""
    dev, ref, gate = dev.double(), ref.double(), torch.as_tensor(gate, dtype=torch.float64)
    assert bool(torch.isfinite(dev).all()), tag
    d = (dev - ref).abs()
    frac = torch.where(d > 0, d / gate.expand_as(d), torch.zeros_like(d))
    i = int(frac.argmax())
    f, e, g = float(frac.reshape(-1)[i]), float(d.reshape(-1)[i]), float(gate.expand_as(d).reshape(-1)[i])
    print("MEASURE %s err=%.3g gate=%.3g frac=%.3g" % (tag, e, g, f))
    assert f <= 1.0, "%s: error %.3g over the gate %.3g" % (tag, e, g)


def _routes(shape, C):
    n1max = R.ALL_SHAPES[shape][0]
    r = [("default", {})]
    if n1max <= 256:
        r.append(("form0", dict(gnn_form=0)))
    if C == 17:
        r += [("sweeps2", dict(gnn_sweeps=2)), ("sweeps3", dict(gnn_sweeps=3))]
    return r + [("sc1", dict(gnn_store_sc1=1))]


@functools.lru_cache(maxsize=None)
def _dev_graphs(shape, pairs=None):
    """Device CSR tensors of a box; ``pairs``: a tuple of pair indices to keep (re-based CSR)."""
    cpu, l1, l2 = R._graphs(shape)
    if pairs is not None:
        n1max, n2max, n1s, n2s = R.ALL_SHAPES[shape]
        ptr1, nbr1 = R._csr([l1[b] for b in pairs], n1max)
        ptr2, nbr2 = R._csr([l2[b] for b in pairs], n2max)
        cpu = (ptr1, nbr1, ptr2, nbr2, torch.tensor([n1s[b] for b in pairs], dtype=torch.int32),
               torch.tensor([n2s[b] for b in pairs], dtype=torch.int32))
    return tuple(t.to(DEV) for t in cpu)


def _launch(shape, C, kind, last, tune, ord2=None, pairs=None):
    """One layer launch on layer_case's inputs: CPU copies of (Xout, z, vpart) with one guard pair
    behind the batch, everything pre-filled with SENT."""
    n1max, n2max, _, _ = R.ALL_SHAPES[shape]
    X, W, cls_w = R.layer_case(shape, C, kind)
    if pairs is not None:
        X = X[list(pairs)]
    B = X.shape[0]
    ptr1, nbr1, ptr2, nbr2, n1, n2 = _dev_graphs(shape, pairs)
    assert W.numel() == _lib.load().fpm_gnn_param_count(C)
    Xo = torch.full((B + 1, 17, n2max, n1max), SENT, device=DEV)
    z = torch.full((B + 1, n2max, n1max), SENT, device=DEV)
    vp = torch.full((B + 1, n2max, n1max), SENT, device=DEV) if last else None
    with _tuning(**tune):
        ops.gnn_layer(X.to(DEV), C, B, n1max, n2max, (ptr1.data_ptr(), nbr1.data_ptr()),
                      (ptr2.data_ptr(), nbr2.data_ptr()), n1, n2, W.to(DEV), Xo[:B], z[:B],
                      vpart=vp[:B] if last else None, cls_w=cls_w.to(DEV) if last else None,
                      ord2=ord2.to(DEV) if ord2 is not None else None)
        torch.cuda.synchronize()
    return Xo.cpu(), z.cpu(), vp.cpu() if last else None


def _check_layer(tag, out, refs, W, C, cls_w, last):
    """Gate A on one launch's outputs against per-pair references (x1, z, S, K)."""
    Xo, z, vp = out
    B = len(refs)
    w = R.unpack(W, C)
    wc, bc = w["wc"].double(), w["bc"].double()
    assert bool((Xo[B] == SENT).all()) and bool((z[B] == SENT).all()), tag + ": guard pair written"
    assert bool((Xo[:B, 16] == SENT).all()), tag + ": channel 16 written"
    x1d = Xo[:B, :16].reshape(B, 16, -1).transpose(1, 2).double()          # (B, N, 16)
    zd = z[:B].reshape(B, -1).double()
    x1r = torch.stack([r[0] for r in refs])
    zr = torch.stack([r[1] for r in refs])
    S1 = torch.stack([r[2]["x1"] for r in refs])
    Sz = torch.stack([r[2]["z"] for r in refs])
    K = torch.stack([r[3] for r in refs])
    _gate(tag + " z", zd, zr, (K + 17) * U * Sz)
    if last:
        assert bool((Xo == SENT).all()), tag + ": Xout written by the last form"
        assert bool((vp[B] == SENT).all()), tag + ": guard pair written"
        cw = cls_w[:16].double()
        _gate(tag + " vpart", vp[:B].reshape(B, -1), x1r @ cw, (K + 16) * U * (S1 @ cw.abs()))
    else:
        _gate(tag + " x1", x1d, x1r, K[:, :, None] * U * S1)
        _gate(tag + " z_own", zd, x1d @ wc + bc, 17 * U * (x1d.abs() @ wc.abs() + bc.abs()))


def _layer_all_routes(shape, C, last, kind="rand"):
    X, W, cls_w = R.layer_case(shape, C, kind)
    refs = R.layer_reference(shape, C, kind)
    for route, tune in _routes(shape, C):
        out = _launch(shape, C, kind, last, tune)
        _check_layer("A.%s %s.C%d.%s.%s" % (route, shape, C, "last" if last else "plain", kind), out, refs, W, C,
                     cls_w, last)


# ------------------------------------------------------------------------------- A: layer, every kernel
@pytest.mark.parametrize("last", [False, True], ids=["plain", "last"])
@pytest.mark.parametrize("C", [1, 17])
@pytest.mark.parametrize("shape", BOXES)
def test_layer_vs_float64(shape, C, last):
    """Every route of the box (default, gnn_form 0, gnn_sweeps 2 / 3, gnn_store_sc1) against the
    float64 layer at all n1max * n2max positions of every pair."""
    _layer_all_routes(shape, C, last)


@pytest.mark.parametrize("last", [False, True], ids=["plain", "last"])
@pytest.mark.parametrize("C", [1, 17])
def test_layer_vs_float64_init_weights(C, last):
    """The same with the model's own initial weights (init_params(7): layer 0 at C = 1, layer 1 at 17)."""
    _layer_all_routes("40x24", C, last, kind="init")


@pytest.mark.parametrize("last", [False, True], ids=["plain", "last"])
@pytest.mark.parametrize("C", [1, 17])
def test_layer_vs_float64_1024(C, last):
    """The ABI's cap, 1024 threads per block; at C = 17 the launch with 80 KiB of dynamic LDS."""
    _layer_all_routes("1024x16", C, last)


# --------------------------------------------------------------------- B: schedule and composition
def _equal(tag, a, r):
    for name, x, y in zip(("Xout", "z", "vpart"), a, r):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y), "%s: %s differs" % (tag, name)


@pytest.mark.parametrize("last", [False, True], ids=["plain", "last"])
@pytest.mark.parametrize("C", [1, 17])
@pytest.mark.parametrize("shape", ["16x12x9", "257x24"])
def test_ord2_is_a_schedule_only(shape, C, last):
    """A random block order of the graph-2 nodes gives bit-equal outputs."""
    n1max, n2max, n1s, _ = R.ALL_SHAPES[shape]
    g = torch.Generator().manual_seed(n1max + C)
    ord2 = torch.stack([torch.randperm(n2max, generator=g) for _ in n1s]).to(torch.int32)
    assert not torch.equal(ord2[0], torch.arange(n2max, dtype=torch.int32))
    _equal("ord2 %s" % shape, _launch(shape, C, "rand", last, {}, ord2=ord2), _launch(shape, C, "rand", last, {}))


@pytest.mark.parametrize("last", [False, True], ids=["plain", "last"])
@pytest.mark.parametrize("C", [1, 17])
@pytest.mark.parametrize("shape,b", [("16x12x9", 3), ("16x12x9", 8), ("257x24", 1)])
def test_pair_alone_equals_its_slice(shape, b, C, last):
    """Pair b re-run alone in the same box (its CSR re-based to 0) is bit-equal to its slice of the
    batch: 16x12x9 pair 8 is the second round of the pair-to-XCD mapping."""
    whole = _launch(shape, C, "rand", last, {})
    alone = _launch(shape, C, "rand", last, {}, pairs=(b,))
    _equal("pair %d of %s" % (b, shape), tuple(None if t is None else t[0] for t in alone),
           tuple(None if t is None else t[b] for t in whole))


# ---------------------------------------------------------------------------------------- C: readout
@pytest.mark.parametrize("with_vpart", [False, True], ids=["full", "vpart"])
@pytest.mark.parametrize("n1max,n2max", [(64, 64), (65, 63), (13, 130), (130, 13)])
def test_readout_vs_float64(n1max, n2max, with_vpart):
    """ops.node_classifier over the whole box of three pairs against ref_readout; the shapes sit on
    the edges of the 64 x 64 transposed tiles in both directions."""
    B = 3
    g = torch.Generator().manual_seed(n1max * 3 + n2max)
    X = torch.randn(B, 17, n2max, n1max, generator=g)
    w, bias = torch.randn(17, generator=g), torch.randn(1, generator=g)
    vp = torch.randn(B, n2max, n1max, generator=g) if with_vpart else None
    s = torch.full((B + 1, n1max, n2max), SENT, device=DEV)
    ops.node_classifier(X.to(DEV), B, n1max, n2max, w.to(DEV), bias.to(DEV), s[:B],
                        vpart=vp.to(DEV) if with_vpart else None)
    torch.cuda.synchronize()
    s = s.cpu()
    ref, S = R.ref_readout(X, w, bias, vp)
    assert bool((s[B] == SENT).all()), "guard pair written"
    _gate("C.%s %dx%d" % ("vpart" if with_vpart else "full", n1max, n2max), s[:B], ref, (3 if with_vpart else 19) * U * S)


# ------------------------------------------------------------------------------------------ D: chain
def _device_chain(shape, X0, Ws, cls_w, cls_b, ord2):
    """Three layers, their Sinkhorns and the readout exactly as Net issues them (strided channel-16
    output view, vpart on the last layer): CPU copies of the three Xn, the three z, vpart and s."""
    n1max, n2max, n1s, _ = R.ALL_SHAPES[shape]
    B = len(n1s)
    ptr1, nbr1, ptr2, nbr2, n1, n2 = _dev_graphs(shape)
    csr1, csr2 = (ptr1.data_ptr(), nbr1.data_ptr()), (ptr2.data_ptr(), nbr2.data_ptr())
    zbuf = torch.full((B, n2max, n1max), SENT, device=DEV)
    vpart = torch.full((B, n2max, n1max), SENT, device=DEV)
    X, Cin, Xs, zs = X0.to(DEV), 1, [], []
    for l in range(config.GNN_LAYER):
        Xn = torch.full((B, 17, n2max, n1max), SENT, device=DEV)
        last = l == config.GNN_LAYER - 1
        ops.gnn_layer(X, Cin, B, n1max, n2max, csr1, csr2, n1, n2, Ws[l].to(DEV), Xn, zbuf,
                      vpart=vpart if last else None, cls_w=cls_w.to(DEV) if last else None, ord2=ord2)
        ops.sinkhorn(zbuf.transpose(1, 2), n1, n2, config.GNN_SK_ITER, config.SK_TAU, True,
                     out=Xn[:, 16].transpose(1, 2))
        torch.cuda.synchronize()
        Xs.append(Xn.cpu())
        zs.append(zbuf.cpu())
        X, Cin = Xn, 17
    s = torch.full((B, n1max, n2max), SENT, device=DEV)
    ops.node_classifier(X, B, n1max, n2max, cls_w.to(DEV), cls_b.to(DEV), s, vpart=vpart)
    torch.cuda.synchronize()
    return Xs, zs, vpart.cpu(), s.cpu()


@pytest.mark.parametrize("shape", CHAIN)
def test_chain(shape):
    """Stage-isolated (gates A and C on the device's own previous outputs) and end to end (s within
    8 x err32 of the float64 oracle chain per pair), init_params(7), ord2 on the box over 256."""
    n1max, n2max, n1s, n2s = R.ALL_SHAPES[shape]
    B = len(n1s)
    sd = R.init_sd()
    Ws = [R.pack_layer(sd, l) for l in range(3)]
    cls_w, cls_b = sd["classifier.weight"].reshape(-1).float(), sd["classifier.bias"].float()
    # the packed layout the reference unpacks is the one Net hands the kernels
    wp = fpm.Net(regression=True, backbone=False, dtype="f32", seed=7).packed(DEV)
    for l in range(3):
        assert torch.equal(wp["gnn%d" % l].cpu(), Ws[l])
    assert torch.equal(wp["cls_w"].cpu(), cls_w) and torch.equal(wp["cls_b"].cpu(), cls_b)
    X0 = R.chain_inputs(shape, 7)
    ord2 = None
    if n1max > 256:
        g = torch.Generator().manual_seed(3)
        ord2 = torch.stack([torch.randperm(n2max, generator=g) for _ in n1s]).to(torch.int32).to(DEV)
    Xs, zs, vp, s = _device_chain(shape, X0, Ws, cls_w, cls_b, ord2)
    _, l1, l2 = R._graphs(shape)
    # stage-isolated: each layer against the float64 layer on the device's own previous output
    Xin, C = X0, 1
    for l in range(3):
        last = l == 2
        assert bool(torch.isfinite(Xs[l][:, 16]).all()) and not bool((Xs[l][:, 16] == SENT).any()), "channel 16"
        refs = []
        for b in range(B):
            x1, z, S = R.ref_layer(R.pair_x(Xin, b), R.edge_index(l1[b]), R.edge_index(l2[b]), n1max, n2max,
                                   n1s[b], n2s[b], Ws[l], C)
            refs.append((x1, z, S, R.roundings(l1[b], l2[b], n1max, n2max, C)))
        tag = "D.layer%d %s" % (l, shape)
        x1r = torch.stack([r[0] for r in refs])
        S1 = torch.stack([r[2]["x1"] for r in refs])
        K = torch.stack([r[3] for r in refs])
        _gate(tag + " z", zs[l].reshape(B, -1), torch.stack([r[1] for r in refs]),
              (K + 17) * U * torch.stack([r[2]["z"] for r in refs]))
        if last:
            assert bool((Xs[l][:, :16] == SENT).all()), "Xout written by the last layer"
            cw = cls_w[:16].double()
            _gate(tag + " vpart", vp.reshape(B, -1), x1r @ cw, (K + 16) * U * (S1 @ cw.abs()))
        else:
            _gate(tag + " x1", Xs[l][:, :16].reshape(B, 16, -1).transpose(1, 2), x1r, K[:, :, None] * U * S1)
        Xin, C = Xs[l], 17
    ref, S = R.ref_readout(Xs[2], cls_w, cls_b, vp)
    _gate("D.readout %s" % shape, s, ref, 3 * U * S)
    # end to end: s against the float64 oracle chain, per pair
    _, s64 = R.oracle_chain(shape, X0, sd, torch.float64)
    _, s32 = R.oracle_chain(shape, X0, sd, torch.float32)
    for b in range(B):
        err32 = float((s32[b].double() - s64[b]).abs().max())
        _gate("D.s %s.b%d" % (shape, b), s[b], s64[b], 8.0 * err32)


# --------------------------------------------------------------------- E: refusals and empty launch
def _refusal_args(C, n1max, n2max, B=1, sentinel=True):
    mk = (lambda *sh: torch.full(sh, SENT, device=DEV)) if sentinel else (lambda *sh: torch.empty(sh, device=DEV))
    X = torch.zeros(B, C, n2max, n1max, device=DEV)
    ptr1 = torch.zeros(B * n1max + 1, dtype=torch.int32, device=DEV)
    ptr2 = torch.zeros(B * n2max + 1, dtype=torch.int32, device=DEV)
    nbr = torch.zeros(1, dtype=torch.int32, device=DEV)
    n1 = torch.full((B,), n1max, dtype=torch.int32, device=DEV)
    n2 = torch.full((B,), n2max, dtype=torch.int32, device=DEV)
    W = torch.zeros(R.param_count(17), device=DEV)
    return dict(X=X, csr1=(ptr1.data_ptr(), nbr.data_ptr()), csr2=(ptr2.data_ptr(), nbr.data_ptr()), n1=n1, n2=n2,
                W=W, Xo=mk(B, 17, n2max, n1max), z=torch.full((B, n2max, n1max), SENT, device=DEV),
                vp=torch.full((B, n2max, n1max), SENT, device=DEV), keep=(ptr1, ptr2, nbr))


def _refused(C, n1max, n2max, vpart=False, cls_w=None, sentinel=True):
    a = _refusal_args(C, n1max, n2max, sentinel=sentinel)
    with pytest.raises(_lib.FpmError):
        ops.gnn_layer(a["X"], C, 1, n1max, n2max, a["csr1"], a["csr2"], a["n1"], a["n2"], a["W"], a["Xo"], a["z"],
                      vpart=a["vp"] if vpart else None, cls_w=cls_w)
    torch.cuda.synchronize()
    assert bool((a["z"] == SENT).all()) and bool((a["vp"] == SENT).all()), "a refused call launched"
    if sentinel:
        assert bool((a["Xo"] == SENT).all()), "a refused call launched"


def test_refusals():
    """C = 2, vpart without cls_w, n1max = 1025 and a pair state of 2 GiB raise FpmError and launch nothing."""
    _refused(2, 16, 12)
    _refused(17, 16, 12, vpart=True, cls_w=None)
    _refused(1, 1025, 9)
    # 17 * 1024 * 30841 * 4 B = 2^31 + 39 KiB: the smallest n2max at n1max = 1024 that is refused (Xout
    # is allocated for real, 2 GiB, and not filled)
    assert 17 * 1024 * 30841 * 4 >= 2 ** 31 > 17 * 1024 * 30840 * 4
    _refused(1, 1024, 30841, sentinel=False)


def test_empty_batch_writes_nothing():
    """B = 0: status 0 and no launch, for the layer and the readout."""
    a = _refusal_args(17, 16, 12)
    ops.gnn_layer(a["X"][:0], 17, 0, 16, 12, a["csr1"], a["csr2"], a["n1"][:0], a["n2"][:0], a["W"], a["Xo"][:0],
                  a["z"][:0], vpart=a["vp"][:0], cls_w=torch.zeros(17, device=DEV))
    s = torch.full((1, 16, 12), SENT, device=DEV)
    ops.node_classifier(a["Xo"][:0], 0, 16, 12, torch.zeros(17, device=DEV), torch.zeros(1, device=DEV), s[:0])
    torch.cuda.synchronize()
    for t in (a["Xo"], a["z"], a["vp"], s):
        assert bool((t == SENT).all())

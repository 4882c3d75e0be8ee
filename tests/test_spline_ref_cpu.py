"""The float64 SplineConv reference of tests/spline_ref.py against the oracle, and the power of the
hand-built batches that tests/test_spline_stages.py runs on the GPU (no GPU needed here).

The batches (``edge_batch``, ``tiny_batch``) are built here and imported by the GPU tests.

Edge batch: 3 graphs (4 in the "empty" version) in boxes of nmax = 100 keypoints.
  graph 0  n = 100, Delaunay (synth.make_graph); the pseudo-coordinates of its first 29 edges (the
           out-edges of nodes 0 .. 5, so the border cells hold 1 to 6 rows) are
           overwritten with every pair from {0, 0.25, 0.5, 0.75, 1}^2 (saturated coordinates:
           floor(4p) = 4, the wrapped cell; exact quarters: a basis corner of exactly 0) and with
           four pairs holding 1.125.  Up to p = 1 the wrapped corner's weight is exactly 0
           (p = 1 -> frac = 0), so a wrong wrap shows in the plan only; 1.125 is inside the range the
           kernels and the reference's ``% kernel_size`` define (floor(4p) = 4, frac = 0.5) and makes
           the wrapped cell carry weight in the output as well.
  graph 1  n = 37, directed and asymmetric, edges in shuffled order: node 0 has 40 in-edges (a
           star, some of them parallel edges), node 1 out-edges only, node 2 in-edges only (all
           three in cell 12's corner), node 3 is valid and isolated, 10 -> 11 exists twice with
           different pseudo-coordinates.
  graph 2  "plain": n = 21 Delaunay; "empty": n = 5 without edges, followed by graph 3 (n = 30).
Rows of padded nodes hold 0.5 (not 0), so a padded row that leaked into an output would show.
"""
import functools
import types

import numpy as np
import pytest
import torch

from fpm import params, synth
import oracle as O

import spline_ref as R

NMAX = 100
QUARTERS = (0.0, 0.25, 0.5, 0.75, 1.0)
OVER = ((1.125, 0.3), (0.6, 1.125), (1.125, 1.125), (1.125, 1.0))
SPL = O.ngm_oracle.SPLINE
NEG_CELL = 12


def _graph1():
    """The directed 37-node graph of the module docstring -> (src, dst, pseudo), shuffled."""
    rng = np.random.default_rng(137)
    e = []
    star = [1] + list(range(4, 37)) + list(range(4, 10))                  # 40 in-edges of node 0
    e += [(u, 0) for u in star]
    e += [(1, 4), (1, 5), (1, 6)]                                         # node 1: out-edges only
    e += [(0, 4), (0, 20)]
    for u in range(4, 37):                                                # 3 random targets each, no reverse pairing
        for v in rng.choice([w for w in range(4, 37) if w != u], size=3, replace=False):
            e.append((u, int(v)))
    e += [(10, 11), (10, 11)]                                             # the duplicated edge
    src = np.array([a for a, _ in e], dtype=np.int64)
    dst = np.array([b for _, b in e], dtype=np.int64)
    pseudo = rng.uniform(0.26, 0.74, (len(e), 2)).astype(np.float32)      # the 4 central groups ...
    pseudo[0] = (1.0, 0.0)                                                # ... but one saturated edge
    into2 = np.array([[0.5, 0.5], [0.55, 0.6], [0.6, 0.5]], dtype=np.float32)   # node 2: in-edges only, cell 12
    src = np.concatenate([src, [7, 8, 9]])
    dst = np.concatenate([dst, [2, 2, 2]])
    pseudo = np.concatenate([pseudo, into2])
    perm = rng.permutation(src.size)
    return src[perm], dst[perm], pseudo[perm]


def _features(rng, n):
    x = rng.standard_normal((n, 768)).astype(np.float32)
    x[:, :256] /= np.linalg.norm(x[:, :256], axis=1, keepdims=True)
    x[:, 256:] /= np.linalg.norm(x[:, 256:], axis=1, keepdims=True)
    return x


def _assemble(graphs, nmax):
    """Graphs (dicts of n, x, src, dst, pseudo with local ids) -> one side-batch: global ids
    b * nmax + local, edges grouped by graph, padded feature rows 0.5."""
    B = len(graphs)
    x = np.full((B * nmax, 768), 0.5, dtype=np.float32)
    src, dst, ps = [], [], []
    for b, gph in enumerate(graphs):
        x[b * nmax:b * nmax + gph["n"]] = gph["x"]
        src.append(gph["src"] + b * nmax)
        dst.append(gph["dst"] + b * nmax)
        ps.append(gph["pseudo"].reshape(-1, 2))
    return types.SimpleNamespace(
        B=B, nmax=nmax, num_nodes=B * nmax, graphs=graphs, x=x, src=np.concatenate(src).astype(np.int64),
        dst=np.concatenate(dst).astype(np.int64), pseudo=np.concatenate(ps).astype(np.float32),
        nvalid=np.array([gph["n"] for gph in graphs], dtype=np.int64),
        max_graph_edges=max(gph["src"].size for gph in graphs))


def _from_synth(seed, p, n):
    gph = synth.make_graph(seed, p, 0, n)
    return dict(n=n, x=gph["x"], src=gph["edge_index"][0].copy(), dst=gph["edge_index"][1].copy(),
                pseudo=gph["pseudo"].copy())


@functools.lru_cache(maxsize=None)
def edge_batch(version):
    """version "plain" (B = 3) or "empty" (B = 4, graph 2 has no edges and is not the last)."""
    g0 = _from_synth(41, 0, 100)
    combos = [(a, b) for b in QUARTERS for a in QUARTERS] + list(OVER)
    assert g0["src"].size > len(combos)
    g0["pseudo"][:len(combos)] = combos                           # a fixed subset: the first edges (few sources)
    s1, d1, p1 = _graph1()
    g1 = dict(n=37, x=_features(np.random.default_rng(237), 37), src=s1, dst=d1, pseudo=p1)
    if version == "plain":
        gs = [g0, g1, _from_synth(41, 2, 21)]
    else:
        e = np.zeros(0, dtype=np.int64)
        g2 = dict(n=5, x=_features(np.random.default_rng(337), 5), src=e, dst=e, pseudo=np.zeros((0, 2), np.float32))
        gs = [g0, g1, g2, _from_synth(41, 3, 30)]
    return _assemble(gs, NMAX)


@functools.lru_cache(maxsize=None)
def tiny_batch(nmax):
    """9 Delaunay graphs of 5 .. nmax keypoints (nmax = 27: the per-graph plan, 25: the global one)."""
    ns = [nmax, 5, 9, nmax - 1, 12, 7, nmax, 16, 6]
    return _assemble([_from_synth(43, p, n) for p, n in enumerate(ns)], nmax)


@functools.lru_cache(maxsize=None)
def init_weights():
    """(sd, W0, b0, W1, b1): init_params(7) and its kernel layout, W (26, 768 out, 768 in) = the 25
    cells transposed then the root weight transposed (what Net.packed builds)."""
    sd = params.init_params(7)
    out = [sd]
    for l in range(2):
        pre = "%s.%d" % (SPL, l)
        W = torch.cat([sd[pre + ".weight"].transpose(1, 2), sd[pre + ".root"].t()[None]]).contiguous().float()
        out += [W.numpy(), sd[pre + ".bias"].float().numpy()]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def negative_cell_weights(version):
    """Random W (26, 768, 768) and bias whose cell-12 products are negative for every node of the
    edge batch: W[12] = R - a u^T with X u = 1 for the batch's feature rows X (they are linearly
    independent: fewer rows than channels) and a in [0.5, 1.5]."""
    bt = edge_batch(version)
    rng = np.random.default_rng(12)
    W = (rng.standard_normal((26, 768, 768)) * 0.05).astype(np.float32)
    u = np.linalg.pinv(bt.x.astype(np.float64)) @ np.ones(bt.num_nodes)
    a = rng.uniform(0.5, 1.5, 768)
    W[NEG_CELL] = (W[NEG_CELL].astype(np.float64) - np.outer(a, u)).astype(np.float32)
    bias = (rng.standard_normal(768) * 0.05).astype(np.float32)
    return W, bias


def oracle_sd(W0, b0, W1, b1, dtype):
    """Kernel-layout weights -> the oracle's state-dict entries ([cell][in][out], root [in][out])."""
    sd = {}
    for l, (W, b) in enumerate(((W0, b0), (W1, b1))):
        Wt = torch.from_numpy(np.asarray(W)).to(dtype)
        sd["%s.%d.weight" % (SPL, l)] = Wt[:25].transpose(1, 2).contiguous()
        sd["%s.%d.root" % (SPL, l)] = Wt[25].t().contiguous()
        sd["%s.%d.bias" % (SPL, l)] = torch.from_numpy(np.asarray(b)).to(dtype)
    return sd


def _graph_tensors(gph, dtype):
    return (torch.from_numpy(gph["x"]).to(dtype), torch.from_numpy(np.stack([gph["src"], gph["dst"]])),
            torch.from_numpy(gph["pseudo"]))


def weights_of(kind, version):
    """(W0, b0, W1, b1): "init" = init_params(7); "negcell" = negative_cell_weights in both layers."""
    if kind == "init":
        return init_weights()[1:]
    W, b = negative_cell_weights(version)
    return W, b, W, b


@functools.lru_cache(maxsize=None)
def oracle_sconv(version, dtype, kind="init"):
    """oracle.siamese_sconv per graph of the edge batch -> list of (n, 768) float64 arrays."""
    bt = edge_batch(version)
    W0, b0, W1, b1 = weights_of(kind, version)
    sd = oracle_sd(W0, b0, W1, b1, dtype)
    return [O.siamese_sconv(*_graph_tensors(gph, dtype), sd).double().numpy() for gph in bt.graphs]


@functools.lru_cache(maxsize=None)
def stage_d_gate(version, kind="init"):
    """The fp32 gate of the chained-layers stage: max(2e-5, 8 * err32), err32 = the fp32 oracle
    against the float64 oracle on the same graphs."""
    o64, o32 = oracle_sconv(version, torch.float64, kind), oracle_sconv(version, torch.float32, kind)
    err32 = max(float(np.abs(a - b).max()) for a, b in zip(o64, o32))
    return max(2e-5, 8.0 * err32), err32


@functools.lru_cache(maxsize=None)
def ref_plan_of(version):
    bt = edge_batch(version)
    return R.ref_plan(bt.src, bt.dst, bt.pseudo, bt.num_nodes, bt.nmax)


def _valid_rows(bt):
    return np.concatenate([np.arange(gph["n"]) + b * bt.nmax for b, gph in enumerate(bt.graphs)])


# float64 dot products of 768 terms, summed in another order by the oracle's one wide matmul than by
# the reference's per-cell ones: 768 * 2^-53 of the magnitude sum, twice for two layers
F64_GATE = 2 * 768 * 2.0 ** -53


# ---------------------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("version", ["plain", "empty"])
def test_edge_batch_holds_its_cases(version):
    bt = edge_batch(version)
    pl = ref_plan_of(version)
    E0 = bt.graphs[0]["src"].size
    p0 = bt.pseudo[:E0]
    for a in QUARTERS:
        for b in QUARTERS:
            assert ((p0[:, 0] == a) & (p0[:, 1] == b)).any(), (a, b)
    f = np.floor(bt.pseudo * np.float32(4))
    assert (f == 4).any(axis=0).all()                                     # both wraps are used
    assert (pl["basis"] == 0).any() and (pl["basis"] == 1).any()
    indeg = np.diff(pl["dst_ptr"])
    outdeg = np.bincount(bt.src, minlength=bt.num_nodes)
    g1 = bt.nmax
    assert indeg[g1] == 40
    assert indeg[g1 + 1] == 0 and outdeg[g1 + 1] > 0
    assert indeg[g1 + 2] == 3 and outdeg[g1 + 2] == 0 and pl["mask"][g1 + 2] == 1 << 25
    assert indeg[g1 + 3] == 0 and outdeg[g1 + 3] == 0
    pairs = bt.src * bt.num_nodes + bt.dst
    assert np.unique(pairs).size < pairs.size                             # parallel edges
    s1 = bt.src[E0:E0 + bt.graphs[1]["src"].size]
    assert (np.diff(s1) < 0).any()                                        # shuffled inside the graph
    und = set(zip(bt.graphs[1]["src"].tolist(), bt.graphs[1]["dst"].tolist()))
    assert any((b, a) not in und for a, b in und)                         # asymmetric
    sizes = np.diff(pl["cell_off"])
    assert sizes[25] == bt.num_nodes and bt.num_nodes > 256
    assert (sizes[:25] % 128 != 0).sum() > 12 and (sizes[:25] <= 1).any()
    if version == "empty":
        assert bt.graphs[2]["src"].size == 0 and bt.B == 4 and bt.graphs[3]["src"].size > 0
        assert (pl["mask"][2 * bt.nmax:3 * bt.nmax] == 1 << 25).all()


@pytest.mark.parametrize("nmax", [27, 25])
def test_tiny_batch_shape(nmax):
    bt = tiny_batch(nmax)
    assert bt.B == 9 and bt.nvalid.max() == nmax and bt.nvalid.min() == 5


# ------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("version", ["plain", "empty"])
def test_ref_plan_basis_equals_oracle(version):
    bt = edge_batch(version)
    pl = ref_plan_of(version)
    basis, wi = O.spline_basis(torch.from_numpy(bt.pseudo))
    assert np.array_equal(basis.numpy().view(np.uint32), pl["basis"].view(np.uint32))
    assert np.array_equal(wi.numpy(), pl["cells"])
    assert np.array_equal(pl["g"], pl["cells"][:, 0])


@pytest.mark.parametrize("version", ["plain", "empty"])
@pytest.mark.parametrize("weights", ["init", "negcell"])
def test_ref_layer_equals_oracle_spline_conv(version, weights):
    """One layer, both modes, per graph against oracle.spline_conv in float64."""
    bt = edge_batch(version)
    pl = ref_plan_of(version)
    if weights == "init":
        _, W, b, _, _ = init_weights()
    else:
        W, b = negative_cell_weights(version)
    sd = oracle_sd(W, b, W, b, torch.float64)
    out0, S0 = R.ref_layer(bt.x, pl, W, b, 0, None, bt.nvalid)
    out1, S1 = R.ref_layer(bt.x, pl, W, b, 1, bt.x, bt.nvalid)
    clipped = False
    for i, gph in enumerate(bt.graphs):
        x, ei, ps = _graph_tensors(gph, torch.float64)
        o = O.spline_conv(x, ei, ps, sd[SPL + ".0.weight"], sd[SPL + ".0.root"], sd[SPL + ".0.bias"])
        rows = slice(i * bt.nmax, i * bt.nmax + gph["n"])
        for got, S, ref in ((out0, S0, torch.relu(o)), (out1, S1, x + 0.1 * o)):
            d = np.abs(got[rows] - ref.numpy())
            assert (d <= F64_GATE * S[rows]).all(), float((d / S[rows]).max())
        assert (out0[i * bt.nmax + gph["n"]:(i + 1) * bt.nmax] == 0).all()
        assert (out1[i * bt.nmax + gph["n"]:(i + 1) * bt.nmax] == 0).all()
        clipped |= bool((o < 0).any())
    if weights == "negcell":
        Y = R.ref_products(bt.x, pl, W)
        off = pl["cell_off"]
        assert off[NEG_CELL + 1] - off[NEG_CELL] > 50 and (Y[off[NEG_CELL]:off[NEG_CELL + 1]] < 0).all()
        msg, _ = R.ref_messages(Y, pl)
        v = bt.nmax + 2                                                   # graph 1's in-only node
        assert (msg[pl["dst_ptr"][v]:pl["dst_ptr"][v + 1]].max(axis=0) < 0).sum() > 384   # negative maxima
        assert clipped


@pytest.mark.parametrize("version", ["plain", "empty"])
@pytest.mark.parametrize("kind", ["init", "negcell"])
def test_ref_sconv_equals_oracle_siamese(version, kind):
    bt = edge_batch(version)
    W0, b0, W1, b1 = weights_of(kind, version)
    out, S = R.ref_sconv(bt.x, ref_plan_of(version), W0, b0, W1, b1, bt.nvalid)
    for i, (gph, ref) in enumerate(zip(bt.graphs, oracle_sconv(version, torch.float64, kind))):
        rows = slice(i * bt.nmax, i * bt.nmax + gph["n"])
        d = np.abs(out[rows] - ref)
        assert (d <= F64_GATE * S[rows]).all(), float((d / S[rows]).max())


# --------------------------------------------------------------------------- the power of the inputs
@pytest.mark.parametrize("variant", ["swap12", "clamp", "empty_neginf", "empty_root", "drop_last"])
def test_deliberate_change_moves_the_output(variant):
    """Each mistake of spline_ref's ``variant`` list, applied to the reference on the edge batch,
    moves the chained output by >= 100 x the fp32 gate of the chained-layers stage.  ("empty_neginf"
    also has to move layer 0's output -- ReLU turns the -inf into 0 there -- by as much: layer 1's
    then is -inf.)  The weights are the random ones: with init_params(7) (weights of std 0.004) the
    two layers together move x by 1.2e-3 at the most, less than 100 x the 2e-5 floor of the gate, so
    no mistake at all could move that output far enough (measured there: swap12 5e-4, clamp 3e-4,
    drop_last 3e-4); the stage tests run both sets of weights."""
    version = "empty"
    bt = edge_batch(version)
    W0, b0, W1, b1 = weights_of("negcell", version)
    gate, err32 = stage_d_gate(version, "negcell")
    rows = _valid_rows(bt)
    good, _ = R.ref_sconv(bt.x, ref_plan_of(version), W0, b0, W1, b1, bt.nvalid)
    plan_level = variant in ("swap12", "clamp")
    pl = R.ref_plan(bt.src, bt.dst, bt.pseudo, bt.num_nodes, bt.nmax, variant) if plan_level else ref_plan_of(version)
    if variant == "empty_neginf":
        h0, _ = R.ref_layer(bt.x, pl, W0, b0, 0, None, bt.nvalid)
        h1, _ = R.ref_layer(bt.x, pl, W0, b0, 0, None, bt.nvalid, variant=variant)
        moved = float(np.abs(h1 - h0)[rows].max())
        bad, _ = R.ref_sconv(bt.x, pl, W0, b0, W1, b1, bt.nvalid, variant=variant)
        assert np.isinf(bad[rows]).any()
    else:
        bad, _ = R.ref_sconv(bt.x, pl, W0, b0, W1, b1, bt.nvalid, variant=None if plan_level else variant)
        moved = float(np.abs(bad - good)[rows].max())
    print("MEASURE power.%s moved=%.3g gate=%.3g err32=%.3g ratio=%.3g" % (variant, moved, gate, err32, moved / gate))
    assert moved >= 100.0 * gate

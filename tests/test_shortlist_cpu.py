"""Shortlisted 1:N identification, host side (no GPU): ``ops.coarse_score`` on CPU tensors (the
statement of the coarse score) against the definition assembled from the oracle's pieces, and the
host path of ``ops.rank_select`` against a numpy sort on the ranking key and ``ops.rank_topk``.

The helpers here (case shapes, rows, coefficients, the oracle-side definition) also serve
``test_shortlist_gpu.py``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle.ngm_oracle as O
from fpm import _lib, ops, params, synth

# (n0, n_g): square, transposed (n0 > n_g), dummy rows (n0 < n_g), single rows / columns, tile edges
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 5), (5, 2), (17, 16), (33, 64), (128, 1), (100, 127), (128, 128)]
PROBE_NS = sorted({a for a, _ in SHAPES})
ENTRY_NS = sorted({b for _, b in SHAPES})


def state_dicts():
    """init_params(7) (Kp nearly constant at 0.19) and the same with A.bias = 2.0 (Kp over [0.05, 1.6])."""
    sd = params.init_params(7)
    sd2 = {k: v.clone() for k, v in sd.items()}
    sd2["vertex_affinity.A.bias"] = torch.full_like(sd["vertex_affinity.A.bias"], 2.0)
    return {"flat": sd, "spread": sd2}


def graph_rows(g, sd):
    """A graph's SplineConv output rows (n, 768) fp32 from the oracle."""
    return O.siamese_sconv(torch.from_numpy(g["x"]), torch.from_numpy(g["edge_index"]),
                           torch.from_numpy(g["pseudo"]), sd).contiguous()


def coefficients(wp, wg, sd):
    """c = tanh(A normalize(cat(w_p, w_g)) + b) per entry, fp32 (B, 768)."""
    gw = O.global_weights(torch.from_numpy(wp)[None].expand(len(wg), -1), torch.from_numpy(np.stack(wg)))
    return torch.tanh(F.linear(gw, sd["vertex_affinity.A.weight"], sd["vertex_affinity.A.bias"])).contiguous()


def definition64(yp, coef_b, yg):
    """The coarse score of one pair from the oracle's pieces, fp64 arithmetic on the bf16 operands."""
    a = (yp * coef_b).to(torch.bfloat16).double()
    b = yg.to(torch.bfloat16).double()
    Kp = F.softplus(a @ b.t()) - 0.5
    n0, ng = Kp.shape
    P = O.pygm_sinkhorn(Kp[None], [n0], [ng], dummy_row=True, max_iter=10, tau=0.01)[0]
    return float((P * Kp).sum() / min(n0, ng))


def ragged_case(sd, seed=42):
    """Entries of every ENTRY_NS size (one ragged index) and probes of every PROBE_NS size:
    (y, row_off, entry globals, [(yp, w_p)])."""
    entries = [synth.make_graph(seed, p, 1, n) for p, n in enumerate(ENTRY_NS)]
    probes = [synth.make_graph(seed, p, 0, n) for p, n in enumerate(PROBE_NS)]
    rows = [graph_rows(g, sd) for g in entries]
    row_off = torch.tensor(np.concatenate([[0], np.cumsum(ENTRY_NS)]), dtype=torch.int64)
    return torch.cat(rows), row_off, [g["w"] for g in entries], [(graph_rows(g, sd), g["w"]) for g in probes]


@pytest.mark.parametrize("name", ["flat", "spread"])
def test_coarse_score_host_is_the_definition(name):
    sd = state_dicts()[name]
    y, row_off, wg, probes = ragged_case(sd)
    idx = torch.tensor(list(range(len(ENTRY_NS))) + [2], dtype=torch.int32)      # one entry twice
    seen = set()
    for (yp, wp), n0 in zip(probes, PROBE_NS):
        coef = coefficients(wp, [wg[i] for i in idx.tolist()], sd)
        got = ops.coarse_score(y, row_off, idx, yp, coef, dtype=torch.float64)
        assert got.dtype == torch.float64 and tuple(got.shape) == (idx.numel(),)
        for b, g in enumerate(idx.tolist()):
            ref = definition64(yp, coef[b], y[int(row_off[g]):int(row_off[g + 1])])
            assert abs(float(got[b]) - ref) <= 1e-12, (n0, ENTRY_NS[g], float(got[b]), ref)
            seen.add((n0, ENTRY_NS[g]))
        assert float(got[2]) == float(got[-1])
        got32 = ops.coarse_score(y, row_off, idx, yp, coef)
        assert got32.dtype == torch.float32
        assert float((got32.double() - got).abs().max()) < 1e-5
    assert set(SHAPES) <= seen


def test_coarse_score_host_refusals():
    y = torch.zeros(140, 768)
    row_off = torch.tensor([0, 3, 132, 140], dtype=torch.int64)
    yp, coef = torch.zeros(4, 768), torch.zeros(2, 768)
    idx = torch.tensor([0, 2], dtype=torch.int32)
    ops.coarse_score(y, row_off, idx, yp, coef)
    with pytest.raises(_lib.FpmError, match="idx must be a int32"):
        ops.coarse_score(y, row_off, idx.long(), yp, coef)
    with pytest.raises(_lib.FpmError, match="contiguous"):
        ops.coarse_score(y, row_off, torch.stack([idx, idx], 1)[:, 0], yp, coef)
    with pytest.raises(_lib.FpmError, match="outside"):
        ops.coarse_score(y, row_off, torch.tensor([0, 3], dtype=torch.int32), yp, coef)
    with pytest.raises(_lib.FpmError, match="COARSE_NMAX"):
        ops.coarse_score(y, row_off, torch.tensor([0, 1], dtype=torch.int32), yp, coef)
    with pytest.raises(_lib.FpmError, match="COARSE_NMAX"):
        ops.coarse_score(y, row_off, idx, torch.zeros(129, 768), coef)
    with pytest.raises(_lib.FpmError, match="coef"):
        ops.coarse_score(y, row_off, idx, yp, torch.zeros(3, 768))


# ------------------------------------------------------------------------------------ rank_select
def _key_numpy(s):
    """The ranking key restated in numpy: (order-preserving bits) << 32 | (0xFFFFFFFF - index)."""
    s = np.asarray(s, dtype=np.float32)
    u = s.view(np.uint32).astype(np.uint64)
    bits = np.where(u >> np.uint64(31) != 0, np.uint64(0xFFFFFFFF) - u, u | np.uint64(0x80000000))
    bits = np.where(np.isnan(s), np.uint64(0), bits)
    i = np.arange(s.shape[-1], dtype=np.uint64)
    return (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - i)


def rank_scores(P, G, seed):
    """Every value twice, many-way ties, NaNs, infinities and signed zeros."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(P, G, generator=g)
    h = G // 2
    s[:, G - h:] = s[:, :h].flip(1)
    if G > 8:
        s[:, 8:] = s[:, 8:].round(decimals=1)
        s[:, 3] = float("nan")
        s[:, G - 2] = float("nan")
        s[0, 5], s[0, 6] = float("inf"), float("-inf")
        s[-1, 5], s[-1, 6] = 0.0, -0.0
    return s


@pytest.mark.parametrize("P,G,k", [(3, 300, 7), (2, 5, 5), (1, 1, 1), (2, 1000, 129), (2, 3000, 1024), (1, 1500, 1500 - 476)])
def test_rank_select_host_vs_numpy(P, G, k):
    s = rank_scores(P, G, 7 * G + k)
    ti, ts = ops.rank_select(s, k)
    key = _key_numpy(s.numpy())
    order = np.argsort(np.uint64(0xFFFFFFFFFFFFFFFF) - key, axis=1, kind="stable")[:, :k]
    assert ti.dtype == torch.int32 and tuple(ti.shape) == (P, k)
    assert np.array_equal(ti.numpy(), order.astype(np.int32))
    assert np.array_equal(ts.numpy().view(np.uint32), np.take_along_axis(s.numpy(), order, 1).view(np.uint32))
    if k <= 128:
        ri, rs = ops.rank_topk(s, k)
        assert torch.equal(ti, ri) and torch.equal(ts.view(torch.int32), rs.view(torch.int32))


def test_rank_select_equals_rank_topk_at_128():
    s = rank_scores(3, 700, 5)
    a, b = ops.rank_select(s, 128), ops.rank_topk(s, 128)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    wide = torch.zeros(3, 720)
    wide[:, 9:709] = s
    c = ops.rank_select(wide[:, 9:709], 128)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1].view(torch.int32), c[1].view(torch.int32))


def test_rank_select_bad_arguments():
    s = torch.zeros(2, 2000)
    for k in (0, 2001, 1025):
        with pytest.raises(_lib.FpmError, match="rank_select: k"):
            ops.rank_select(s, k)
    with pytest.raises(_lib.FpmError, match="rank_select: k"):
        ops.rank_select(torch.zeros(1, 9), 10)
    with pytest.raises(_lib.FpmError, match="fp32"):
        ops.rank_select(s.double(), 2)
    with pytest.raises(_lib.FpmError, match=r"rank_topk: scores must be a \(P, G\) fp32 tensor"):
        ops.rank_topk([[1.0, 2.0]], 1)

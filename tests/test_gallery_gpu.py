"""Enrolled gallery on the GPU: the cached-row gather kernel against ``rows_bcast_scale`` and a torch
restatement, ``Net.identify`` against the uncached probe x gallery forward (bit for bit), the index
through ``save`` / ``load``, and the device ranking against its host path."""
import numpy as np
import pytest
import torch

import fpm
from fpm import _lib, ops, params, synth
from fpm.batch import DeviceBatch
from fpm.gallery import GalleryIndex

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
OUT_KEYS = ("s", "ss", "ds_mat", "perm_mat", "k_prob", "cls_prob")


@pytest.fixture(scope="module")
def sd():
    return params.init_params(7)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _nan_out(rows, cols, dtype):
    return torch.full((rows, cols), float("nan"), device=DEV, dtype=dtype)


# ------------------------------------------------------------------------------- rows_gather_scale
@pytest.mark.parametrize("with_coef", [True, False])
@pytest.mark.parametrize("dtype,split", [(torch.float32, 0), (torch.bfloat16, 0), (torch.bfloat16, 1),
                                         (torch.bfloat16, 2)])
def test_gather_equals_bcast(dtype, split, with_coef):
    """G = 1, idx = 0, n_0 = nmax: the gather is rows_bcast_scale, bit for bit."""
    g = torch.Generator().manual_seed(21 + split)
    rows, B = 5, 3
    y = torch.randn(rows, 768, generator=g).to(DEV)
    coef = torch.tanh(torch.randn(B, 768, generator=g)).to(DEV) if with_coef else None
    cols = 2304 if split else 768
    ref_f, ref_t = _nan_out(B * rows, 768, torch.float32), _nan_out(B * rows, cols, dtype)
    ops.rows_bcast_scale(y, B, coef=coef, out_f=ref_f, out_t=ref_t, split=split)
    out_f, out_t = _nan_out(B * rows, 768, torch.float32), _nan_out(B * rows, cols, dtype)
    ops.rows_gather_scale(y, torch.tensor([0, rows], dtype=torch.int64, device=DEV),
                          torch.zeros(B, dtype=torch.int32, device=DEV), rows, coef=coef, out_f=out_f, out_t=out_t,
                          split=split)
    assert torch.equal(_bits(out_f), _bits(ref_f))
    assert torch.equal(_bits(out_t), _bits(ref_t))


@pytest.mark.parametrize("dtype,split", [(torch.float32, 0), (torch.bfloat16, 0), (torch.bfloat16, 1),
                                         (torch.bfloat16, 2)])
def test_gather_ragged(dtype, split):
    """Ragged gallery against a torch restatement (index, multiply, bf16 round, hi / lo): valid rows
    bit-equal, padding rows exactly zero in out_f and out_t (outputs pre-filled with NaN)."""
    g = torch.Generator().manual_seed(5)
    n, nmax, idx = [5, 1, 8, 3], 8, [2, 0, 0, 3, 1]
    off = np.concatenate([[0], np.cumsum(n)])
    y = torch.randn(int(off[-1]), 768, generator=g)
    coef = torch.tanh(torch.randn(len(idx), 768, generator=g))
    B, cols = len(idx), 2304 if split else 768
    out_f, out_t = _nan_out(B * nmax, 768, torch.float32), _nan_out(B * nmax, cols, dtype)
    ops.rows_gather_scale(y.to(DEV), torch.as_tensor(off, dtype=torch.int64).to(DEV),
                          torch.tensor(idx, dtype=torch.int32, device=DEV), nmax, coef=coef.to(DEV), out_f=out_f,
                          out_t=out_t, split=split)
    ref_f, z = torch.zeros(B, nmax, 768), torch.zeros(B, nmax, 768)
    for b, gi in enumerate(idx):
        ref_f[b, :n[gi]] = y[off[gi]:off[gi + 1]]
        z[b, :n[gi]] = y[off[gi]:off[gi + 1]] * coef[b]      # fp32 product, rounded once
    if dtype == torch.float32:
        ref_t = z
    else:
        hi = z.to(torch.bfloat16)
        lo = (z - hi.float()).to(torch.bfloat16)
        ref_t = hi if split == 0 else torch.cat([hi, lo, hi] if split == 1 else [hi, hi, lo], dim=-1)
    assert torch.equal(_bits(out_f.cpu()), _bits(ref_f.view(B * nmax, 768)))
    assert torch.equal(_bits(out_t.cpu()), _bits(ref_t.reshape(B * nmax, cols)))
    for b, gi in enumerate(idx):                      # the padding: +0 bits, no NaN left
        assert not _bits(out_f.view(B, nmax, -1)[b, n[gi]:]).any()
        assert not _bits(out_t.view(B, nmax, -1)[b, n[gi]:]).any()


def test_gather_bad_inputs():
    """int64 idx, a non-contiguous idx, idx = G and n_g > nmax raise FpmError and launch nothing (the
    NaN-filled output stays untouched)."""
    n, nmax = [5, 1, 8, 3], 8
    off = torch.as_tensor(np.concatenate([[0], np.cumsum(n)]), dtype=torch.int64).to(DEV)
    y = torch.ones(17, 768, device=DEV)
    out = _nan_out(5 * nmax, 768, torch.float32)
    good = torch.tensor([2, 0, 0, 3, 1], dtype=torch.int32, device=DEV)
    wide = torch.stack([good, good], 1)
    cases = [(good.long(), nmax, out), (wide[:, 0], nmax, out),
             (torch.tensor([2, 0, 4, 3, 1], dtype=torch.int32, device=DEV), nmax, out),
             (good, 7, _nan_out(5 * 7, 768, torch.float32)), (good.cpu(), nmax, out)]
    for idx, nm, o in cases:
        with pytest.raises(_lib.FpmError, match="rows_gather_scale"):
            ops.rows_gather_scale(y, off, idx, nm, out_t=o)
        torch.cuda.synchronize()
        assert bool(torch.isnan(o).all())


# ------------------------------------------------------------------------------------ rank_topk
def _rank_scores(P, G, seed):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(P, G, generator=g)
    h = G // 2
    s[:, G - h:] = s[:, :h].flip(1)                    # every value of the first half twice
    if G > 8:
        s[:, 8:] = s[:, 8:].round(decimals=1)          # many-way ties
        s[:, 3] = float("nan")
        s[:, G - 2] = float("nan")
    return s


@pytest.mark.parametrize("P,G,k", [(3, 300, 7), (2, 5, 5), (2, 1000, 128)])
def test_rank_topk_device_equals_host(P, G, k):
    s = _rank_scores(P, G, 100 + G)
    hi, hs = ops.rank_topk(s, k)
    di, ds = ops.rank_topk(s.to(DEV), k)
    assert di.dtype == torch.int32 and tuple(di.shape) == (P, k)
    assert torch.equal(di.cpu(), hi)
    assert torch.equal(_bits(ds.cpu()), _bits(hs))
    # a strided view (row stride > G)
    wide = torch.zeros(P, G + 9)
    wide[:, 4:4 + G] = s
    vi, vs = ops.rank_topk(wide.to(DEV)[:, 4:4 + G], k)
    assert torch.equal(vi.cpu(), hi) and torch.equal(_bits(vs.cpu()), _bits(hs))


# ------------------------------------------------------------------------------------- identify
def _net(sd, dtype):
    net = fpm.Net(regression=True, backbone=False, dtype=dtype)
    net.load_state_dict(sd)
    return net


CASES = {
    # box <= 64: fp32 SplineConv operands + the fp64 k chain, both net dtypes
    "f32ops-f32": ("f32", 48, [48, 40, 45, 48, 37, 48], "f32"),
    "f32ops-bf16": ("bf16", 48, [48, 40, 45, 48, 37, 48], "f32"),
    # box > 64 on the bf16 net: bf16 SplineConv, split operand rows
    "bf16ops": ("bf16", 72, [72, 65, 70, 51], None),
}


@pytest.fixture(scope="module", params=sorted(CASES))
def enrolled(request, sd):
    dtype, n_probe, ns, sc_mode = CASES[request.param]
    probe = synth.make_graph(40, 0, 0, n_probe)
    gallery = [synth.make_graph(40, p, 1, n) for p, n in enumerate(ns)]
    net = _net(sd, dtype)
    index = net.enroll(gallery, DEV, sc_mode=sc_mode, batch=4)      # two enrolment sub-batches at G = 6
    return net, probe, gallery, index


def _check_rank(res, sel, score="cls_prob"):
    k = int(res["top_idx"].numel())
    hi, hs = ops.rank_topk(res[score].cpu().view(1, -1), k)
    assert torch.equal(res["top_idx"].cpu().long(), torch.as_tensor(sel)[hi[0].long()])
    assert torch.equal(_bits(res["top_score"].cpu()), _bits(hs[0]))


def test_identify_equals_uncached(enrolled):
    """identify over the index = net.run over from_probe_gallery, every output bit for bit; then a
    reordered sub-selection against from_probe_gallery on that sub-list."""
    net, probe, gallery, index = enrolled
    assert index.sc_mode == ("bf16" if max(g["n"] for g in gallery) > 64 else "f32")
    assert index.y.shape == (sum(g["n"] for g in gallery), 768) and index.G == len(gallery)
    ref = net.run(DeviceBatch.from_probe_gallery(probe, gallery, DEV), chunks=2)
    res = net.identify(probe, index, topk=3, chunks=2)
    for k in OUT_KEYS:
        assert torch.equal(res[k], ref[k]), k
    assert set(ref) <= set(res)
    _check_rank(res, list(range(len(gallery))))
    sel = [3, 0, 2]
    ref = net.run(DeviceBatch.from_probe_gallery(probe, [gallery[i] for i in sel], DEV), chunks=2)
    res = net.identify(probe, index, topk=10, select=sel, chunks=2, score="k_prob")
    for k in OUT_KEYS:
        assert torch.equal(res[k], ref[k]), k
    assert res["top_idx"].numel() == 3 and sorted(res["top_idx"].tolist()) == sorted(sel)
    _check_rank(res, sel, "k_prob")


def test_index_save_load_and_stale_weights(enrolled, tmp_path):
    net, probe, gallery, index = enrolled
    path = str(tmp_path / "index.pt")
    index.save(path)
    back = GalleryIndex.load(path, DEV)
    a = net.identify(probe, index, chunks=2)
    b = net.identify([probe], back, chunks=2)[0]
    for k in OUT_KEYS + ("top_idx", "top_score"):
        assert torch.equal(a[k], b[k]), k
    other = _net(params.init_params(8), net.dtype_mode)
    with pytest.raises(_lib.FpmError, match="other SplineConv weights"):
        other.identify(probe, index)
    net2 = _net(params.init_params(7), net.dtype_mode)
    net2.load_state_dict(params.init_params(8))
    with pytest.raises(_lib.FpmError, match="other SplineConv weights"):
        net2.identify(probe, back)


def test_identify_refusals(enrolled):
    net, probe, gallery, index = enrolled
    net.train()
    try:
        with pytest.raises(_lib.FpmError, match="inference only"):
            net.identify(probe, index)
    finally:
        net.eval()
    net.use_graphs = True
    try:
        with pytest.raises(_lib.FpmError, match="eager"):
            net.identify(probe, index)
    finally:
        net.use_graphs = False
    with pytest.raises(_lib.FpmError, match="select"):
        net.identify(probe, index, select=[0, len(gallery)])
    with pytest.raises(_lib.FpmError, match="score"):
        net.identify(probe, index, score="ds_mat")

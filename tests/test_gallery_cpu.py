"""Enrolled gallery, host side (no GPU): the host path of ``ops.rank_topk`` (the statement of the
ranking's semantics), the ``GalleryIndex`` save / load round trip, and the argument checks of
``ops.rows_gather_scale``, which run before the library is called."""
import numpy as np
import pytest
import torch

import fpm
from fpm import _lib, ops
from fpm.gallery import GalleryIndex


def _key_numpy(s):
    """The ranking key restated in numpy: (order-preserving bits) << 32 | (0xFFFFFFFF - index)."""
    s = np.asarray(s, dtype=np.float32)
    u = s.view(np.uint32).astype(np.uint64)
    bits = np.where(u >> np.uint64(31) != 0, np.uint64(0xFFFFFFFF) - u, u | np.uint64(0x80000000))
    bits = np.where(np.isnan(s), np.uint64(0), bits)
    i = np.arange(s.shape[-1], dtype=np.uint64)
    return (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - i)


def _rank_numpy(s, k):
    key = _key_numpy(s)
    # ascending stable sort of the complemented key = descending order of the key
    order = np.argsort(np.uint64(0xFFFFFFFFFFFFFFFF) - key, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(np.asarray(s, dtype=np.float32), order, 1)


def _scores(P, G, seed):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(P, G, generator=g)
    if G > 1:
        h = G // 2
        s[:, G - h:] = s[:, :h].flip(1)                 # every value of the first half twice
        s[:, 1] = s[:, 0]
    if G > 8:
        s[:, 8:] = s[:, 8:].round(decimals=1)           # many-way ties
        s[:, 3] = float("nan")
        s[:, G - 2] = float("nan")
        s[0, 5], s[0, 6] = float("inf"), float("-inf")
        s[1, 5], s[1, 6] = 0.0, -0.0
    return s


@pytest.mark.parametrize("P,G,k", [(3, 300, 7), (2, 5, 5), (1, 1, 1), (4, 130, 128)])
def test_rank_topk_host_vs_numpy(P, G, k):
    s = _scores(P, G, 11 * G + k)
    ti, ts = ops.rank_topk(s, k)
    ri, rs = _rank_numpy(s.numpy(), k)
    assert ti.dtype == torch.int32 and tuple(ti.shape) == (P, k)
    assert np.array_equal(ti.numpy(), ri)
    assert np.array_equal(ts.numpy().view(np.uint32), rs.view(np.uint32))


def test_rank_topk_semantics():
    """Descending; ties to the lower index; NaN after every number, NaNs by index; k = G."""
    nan, inf = float("nan"), float("inf")
    s = torch.tensor([[0.5, nan, 2.0, 0.5, -inf, nan, inf, 2.0]])
    ti, ts = ops.rank_topk(s, 8)
    assert ti.tolist() == [[6, 2, 7, 0, 3, 4, 1, 5]]
    assert ts[0, :6].tolist() == [inf, 2.0, 2.0, 0.5, 0.5, -inf] and bool(torch.isnan(ts[0, 6:]).all())
    # a strided view ranks like its contiguous copy
    wide = torch.randn(3, 40)
    a, b = ops.rank_topk(wide[:, 3:33], 4), ops.rank_topk(wide[:, 3:33].contiguous(), 4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_rank_topk_bad_arguments():
    s = torch.zeros(2, 6)
    for k in (0, 7):
        with pytest.raises(_lib.FpmError, match="rank_topk: k"):
            ops.rank_topk(s, k)
    with pytest.raises(_lib.FpmError, match="rank_topk: k"):
        ops.rank_topk(torch.zeros(1, 200), 129)
    with pytest.raises(_lib.FpmError, match="fp32"):
        ops.rank_topk(s.double(), 2)


def _hand_index(P=True):
    g = torch.Generator().manual_seed(3)
    n = torch.tensor([3, 1, 4], dtype=torch.int32)
    row_off = torch.tensor([0, 3, 4, 8], dtype=torch.int64)
    edge_off = torch.tensor([0, 6, 6, 16], dtype=torch.int64)
    src = torch.randint(0, 3, (16,), generator=g, dtype=torch.int32)
    dst = torch.randint(0, 3, (16,), generator=g, dtype=torch.int32)
    return GalleryIndex(torch.randn(8, 768, generator=g), row_off, n, src, dst, torch.rand(16, 2, generator=g), edge_off,
                        torch.rand(3, 512, generator=g), torch.rand(8, 2, generator=g) if P else None, "f32", 4,
                        "0123abcd")


@pytest.mark.parametrize("with_P", [True, False])
def test_gallery_index_save_load(tmp_path, with_P):
    idx = _hand_index(with_P)
    assert fpm.GalleryIndex is GalleryIndex and idx.G == 3
    assert idx.nbytes() >= 8 * 768 * 4                      # 3 KB per keypoint of rows
    path = str(tmp_path / "gallery.pt")
    idx.save(path)
    # a dict of tensors and scalars: loads with weights_only (no pickled code objects)
    raw = torch.load(path, map_location="cpu", weights_only=True)
    assert isinstance(raw, dict) and all(isinstance(v, (torch.Tensor, str, int)) for v in raw.values())
    back = GalleryIndex.load(path, "cpu")
    for k in ("y", "row_off", "n", "src", "dst", "pseudo", "edge_off", "w"):
        assert torch.equal(getattr(back, k), getattr(idx, k)), k
        assert getattr(back, k).dtype == getattr(idx, k).dtype, k
    assert (back.P is None) == (idx.P is None) and (idx.P is None or torch.equal(back.P, idx.P))
    assert (back.sc_mode, back._pack_gen, back.weights_id) == ("f32", 4, "0123abcd")


def test_gallery_index_rejects_inconsistent_fields():
    idx = _hand_index()
    with pytest.raises(_lib.FpmError, match="inconsistent"):
        GalleryIndex(idx.y[:7], idx.row_off, idx.n, idx.src, idx.dst, idx.pseudo, idx.edge_off, idx.w, None, "f32", 1, "x")
    with pytest.raises(_lib.FpmError, match="sc_mode"):
        GalleryIndex(idx.y, idx.row_off, idx.n, idx.src, idx.dst, idx.pseudo, idx.edge_off, idx.w, None, "fp16", 1, "x")


def test_rows_gather_scale_argument_checks(monkeypatch):
    """dtype, contiguity, range and n_g > nmax are refused on the host, before the library is
    called (the call is replaced by a trap here)."""
    def trap(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", trap)
    y = torch.zeros(17, 768)
    row_off = torch.tensor([0, 5, 6, 14, 17], dtype=torch.int64)
    idx = torch.tensor([2, 0, 0, 3, 1], dtype=torch.int32)
    out = torch.empty(5 * 8, 768)
    with pytest.raises(_lib.FpmError, match="idx must be a int32"):
        ops.rows_gather_scale(y, row_off, idx.long(), 8, out_t=out)
    with pytest.raises(_lib.FpmError, match="row_off must be a int64"):
        ops.rows_gather_scale(y, row_off.int(), idx, 8, out_t=out)
    with pytest.raises(_lib.FpmError, match="idx must be a contiguous"):
        ops.rows_gather_scale(y, row_off, torch.stack([idx, idx], 1)[:, 0], 8, out_t=out)
    with pytest.raises(_lib.FpmError, match=r"outside \[0, 4\)"):
        ops.rows_gather_scale(y, row_off, torch.tensor([2, 4, 0, 3, 1], dtype=torch.int32), 8, out_t=out)
    with pytest.raises(_lib.FpmError, match=r"outside \[0, 4\)"):
        ops.rows_gather_scale(y, row_off, torch.tensor([2, -1, 0, 3, 1], dtype=torch.int32), 8, out_t=out)
    with pytest.raises(_lib.FpmError, match="n_g = 8 > nmax = 7"):
        ops.rows_gather_scale(y, row_off, idx, 7, out_t=torch.empty(5 * 7, 768))
    with pytest.raises(_lib.FpmError, match="shape"):
        ops.rows_gather_scale(y, row_off, idx, 8, out_t=torch.empty(5 * 8, 2304))
    # valid arguments on CPU tensors get as far as the device check: there is no host fallback
    with pytest.raises(_lib.FpmError, match="CPU tensor"):
        ops.rows_gather_scale(y, row_off, idx, 8, out_t=out)

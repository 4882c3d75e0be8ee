"""Compact gallery index, host side (no GPU): the coarse statement on bf16 index rows, ``ops.rows_fetch``
on CPU tensors, the index layouts' constructor checks, byte accounting, ``save`` / ``load`` and the
``fetch`` cap."""
import pytest
import torch

from fpm import _lib, gallery, ops
from fpm.gallery import GalleryIndex
from test_shortlist_cpu import ENTRY_NS, PROBE_NS, SHAPES, coefficients, ragged_case, state_dicts


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ the coarse statement on bf16 rows
_CASE = []


def case():
    """``ragged_case`` of the "spread" weights, computed once and shared (read-only)."""
    if not _CASE:
        sd = state_dicts()["spread"]
        _CASE.append((sd,) + tuple(ragged_case(sd)))
    return _CASE[0]


@pytest.mark.parametrize("op", [ops.coarse_score, ops.coarse_score_wide, ops.coarse_score_stream])
def test_coarse_statement_on_bf16_rows(op):
    """On bf16 rows the statement's rounding is the identity: the same bits as on the fp32 rows."""
    sd, y, row_off, wg, probes = case()
    y16 = y.to(torch.bfloat16)
    idx = torch.tensor(list(range(len(ENTRY_NS))) + [2], dtype=torch.int32)      # one entry twice
    seen = set()
    for (yp, wp), n0 in zip(probes, PROBE_NS):
        coef = coefficients(wp, [wg[i] for i in idx.tolist()], sd)
        ref = op(y, row_off, idx, yp, coef)
        got = op(y16, row_off, idx, yp, coef)
        assert got.dtype == torch.float32 and torch.equal(_bits(got), _bits(ref)), n0
        assert bool(torch.isfinite(got).all())
        seen |= {(n0, ENTRY_NS[g]) for g in idx.tolist()}
    assert set(SHAPES) <= seen


@pytest.mark.parametrize("op", [ops.coarse_score, ops.coarse_score_wide, ops.coarse_score_stream])
def test_coarse_refusals_on_bf16_rows(op):
    y = torch.zeros(11, 768, dtype=torch.bfloat16)
    row_off = torch.tensor([0, 3, 11], dtype=torch.int64)
    yp, coef = torch.zeros(4, 768), torch.zeros(2, 768)
    idx = torch.tensor([0, 1], dtype=torch.int32)
    assert tuple(op(y, row_off, idx, yp, coef).shape) == (2,)
    for bad in (torch.zeros(11, 767, dtype=torch.bfloat16), torch.zeros(11, 1536, dtype=torch.bfloat16)[:, ::2],
                torch.zeros(11, 768, dtype=torch.float16)):
        with pytest.raises(_lib.FpmError, match="y must be contiguous fp32 or bf16 rows of 768 channels"):
            op(bad, row_off, idx, yp, coef)
    # the probe's rows and the coefficients stay fp32
    with pytest.raises(_lib.FpmError, match="yp must be contiguous fp32 rows"):
        op(y, row_off, idx, yp.to(torch.bfloat16), coef)


# --------------------------------------------------------------------------------------- rows_fetch
FETCH_NS = (1, 15, 16, 17, 128)            # both sides of the 16-row band, a single row, several bands


def fetch_case(ns=FETCH_NS, seed=5):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(sum(ns), 768, generator=g)
    row_off = torch.tensor([0] + [sum(ns[:i + 1]) for i in range(len(ns))], dtype=torch.int64)
    return y, row_off


def out_offsets(row_off, idx):
    ng = row_off[idx.long() + 1] - row_off[idx.long()]
    return torch.cat([torch.zeros(1, dtype=torch.int64), ng.cumsum(0)])


@pytest.mark.parametrize("sel", [[4, 0, 2, 0, 3, 1], [3], [0]], ids=["all-one-twice", "M1", "M1-one-row"])
def test_rows_fetch_host(sel):
    y, row_off = fetch_case()
    idx = torch.tensor(sel, dtype=torch.int32)
    off = out_offsets(row_off, idx)
    out = torch.full((int(off[-1]) + 2, 768), float("nan"))
    got = ops.rows_fetch(y, row_off, idx, out, off)
    assert got is out
    want = torch.cat([y[int(row_off[g]):int(row_off[g + 1])] for g in sel])
    assert torch.equal(out[:int(off[-1])], want)
    assert bool(torch.isnan(out[int(off[-1]):]).all())          # nothing past the selection is written


def test_rows_fetch_refusals(monkeypatch):
    def trap(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", trap)
    y, row_off = fetch_case()
    idx = torch.tensor([4, 0, 2], dtype=torch.int32)
    off = out_offsets(row_off, idx)
    out = torch.empty(int(off[-1]), 768)
    ops.rows_fetch(y, row_off, idx, out, off)
    for bad in ([4, 5, 2], [4, -1, 2]):
        with pytest.raises(_lib.FpmError, match=r"idx value outside \[0, 5\)"):
            ops.rows_fetch(y, row_off, torch.tensor(bad, dtype=torch.int32), out, off)
    with pytest.raises(_lib.FpmError, match="out holds 144 rows, the selection has 145"):
        ops.rows_fetch(y, row_off, idx, out[:-1], off)
    with pytest.raises(_lib.FpmError, match="idx must be a int32"):
        ops.rows_fetch(y, row_off, idx.long(), out, off)
    with pytest.raises(_lib.FpmError, match="row_off must be a int64"):
        ops.rows_fetch(y, row_off.int(), idx, out, off)
    with pytest.raises(_lib.FpmError, match="out_off must be a int64"):
        ops.rows_fetch(y, row_off, idx, out, off.int())
    with pytest.raises(_lib.FpmError, match="out_off must hold 4 offsets"):
        ops.rows_fetch(y, row_off, idx, out, off[:-1])
    with pytest.raises(_lib.FpmError, match="out_off must rise"):
        ops.rows_fetch(y, row_off, idx, out, off + 1)
    with pytest.raises(_lib.FpmError, match="src must be contiguous fp32 rows"):
        ops.rows_fetch(y.double(), row_off, idx, out, off)
    with pytest.raises(_lib.FpmError, match="src must be contiguous fp32 rows"):
        ops.rows_fetch(y.to(torch.bfloat16), row_off, idx, out, off)
    with pytest.raises(_lib.FpmError, match="out must be contiguous fp32 rows"):
        ops.rows_fetch(y, row_off, idx, torch.empty(int(off[-1]), 1536)[:, ::2], off)
    with pytest.raises(_lib.FpmError, match="row_off must rise from 0"):
        ops.rows_fetch(y[:-1], row_off, idx, out, off)


# ------------------------------------------------------------------------------------ the container
def hand_index(layout, P=True):
    g = torch.Generator().manual_seed(3)
    n = torch.tensor([3, 1, 4], dtype=torch.int32)
    row_off = torch.tensor([0, 3, 4, 8], dtype=torch.int64)
    edge_off = torch.tensor([0, 6, 6, 16], dtype=torch.int64)
    src = torch.randint(0, 3, (16,), generator=g, dtype=torch.int32)
    dst = torch.randint(0, 3, (16,), generator=g, dtype=torch.int32)
    y = torch.randn(8, 768, generator=g)
    kw = {} if layout == "f32" else dict(y16=y.to(torch.bfloat16), layout=layout)
    return GalleryIndex(y, row_off, n, src, dst, torch.rand(16, 2, generator=g), edge_off,
                        torch.rand(3, 512, generator=g), torch.rand(8, 2, generator=g) if P else None, "f32", 4,
                        "0123abcd", **kw)


@pytest.mark.parametrize("layout", ["bf16+host", "f32+bf16"])
def test_layout_save_load(tmp_path, layout):
    idx = hand_index(layout)
    assert idx.layout == layout and idx.device == torch.device("cpu")
    path = str(tmp_path / "gallery.pt")
    idx.save(path)
    raw = torch.load(path, map_location="cpu", weights_only=True)
    assert isinstance(raw, dict) and all(isinstance(v, (torch.Tensor, str, int)) for v in raw.values())
    assert raw["format"] == 2 and raw["layout"] == layout and raw["y16"].dtype == torch.bfloat16
    back = GalleryIndex.load(path, "cpu")
    for k in ("y", "y16", "row_off", "n", "src", "dst", "pseudo", "edge_off", "w", "P"):
        assert torch.equal(getattr(back, k), getattr(idx, k)), k
        assert getattr(back, k).dtype == getattr(idx, k).dtype, k
    assert (back.layout, back.sc_mode, back._pack_gen, back.weights_id) == (layout, "f32", 4, "0123abcd")
    assert (back.nbytes(), back.host_nbytes()) == (idx.nbytes(), idx.host_nbytes())


def test_f32_layout_still_writes_format_1(tmp_path):
    idx = hand_index("f32")
    assert idx.layout == "f32" and idx.y16 is None and idx.host_nbytes() == 0
    path = str(tmp_path / "gallery.pt")
    idx.save(path)
    raw = torch.load(path, map_location="cpu", weights_only=True)
    assert raw["format"] == 1 and "layout" not in raw and "y16" not in raw
    back = GalleryIndex.load(path, "cpu")
    assert back.layout == "f32" and back.y16 is None and torch.equal(back.y, idx.y)
    raw["format"] = 3
    torch.save(raw, path)
    with pytest.raises(_lib.FpmError, match="not a gallery index of format"):
        GalleryIndex.load(path, "cpu")


def test_byte_accounting():
    f32, both, host = hand_index("f32"), hand_index("f32+bf16"), hand_index("bf16+host")
    numel = f32.y.numel()
    assert host.nbytes() == f32.nbytes() - numel * 2
    assert host.host_nbytes() == numel * 4
    assert both.nbytes() == f32.nbytes() + numel * 2 and both.host_nbytes() == 0


def test_constructor_checks():
    idx = hand_index("f32")
    a = (idx.y, idx.row_off, idx.n, idx.src, idx.dst, idx.pseudo, idx.edge_off, idx.w, None, "f32", 1, "x")
    y16 = idx.y.to(torch.bfloat16)
    for layout in ("f32+bf16", "bf16+host"):
        with pytest.raises(_lib.FpmError, match="inconsistent"):
            GalleryIndex(*a, y16=y16[:7], layout=layout)                         # wrong shape
        with pytest.raises(_lib.FpmError, match="inconsistent"):
            GalleryIndex(*a, y16=idx.y.to(torch.float16), layout=layout)         # wrong dtype
        with pytest.raises(_lib.FpmError, match="needs y16"):
            GalleryIndex(*a, layout=layout)
    with pytest.raises(_lib.FpmError, match="has no y16"):
        GalleryIndex(*a, y16=y16)
    with pytest.raises(_lib.FpmError, match="layout must be one of"):
        GalleryIndex(*a, y16=y16, layout="bf16")


def test_fetch_and_its_cap(monkeypatch):
    idx = hand_index("bf16+host")
    ys, off_d, off_h = idx.fetch(torch.tensor([2, 0, 2]))
    assert torch.equal(ys, torch.cat([idx.y[4:8], idx.y[0:3], idx.y[4:8]]))
    assert off_h.tolist() == [0, 4, 7, 11] and torch.equal(off_d, off_h) and off_h.dtype == torch.int64
    buf = ys.data_ptr()
    ys2, _, off2 = idx.fetch([1])                                   # the staging buffer is reused
    assert ys2.data_ptr() == buf and torch.equal(ys2, idx.y[3:4]) and off2.tolist() == [0, 1]
    assert gallery.FETCH_MAX_BYTES == ops.RANK_SELECT_KMAX * ops.COARSE_STREAM_NMAX * 3072
    monkeypatch.setattr(gallery, "FETCH_MAX_BYTES", 7 * 3072)
    assert tuple(idx.fetch([0, 2])[0].shape) == (7, 768)            # exactly at the cap
    with pytest.raises(_lib.FpmError, match="shortlist="):
        idx.fetch([0, 1, 2])
    with pytest.raises(_lib.FpmError, match=r"entries in \[0, 3\)"):
        idx.fetch([3])
    with pytest.raises(_lib.FpmError, match="holds its fp32 rows on the device"):
        hand_index("f32").fetch([0])

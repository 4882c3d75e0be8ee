"""The streamed coarse score (boxes of up to 600 keypoints, every graph the matcher takes), host side
(no GPU): ``ops.coarse_score_stream`` on CPU tensors against the definition assembled from the
oracle's pieces on shapes up to the full box, its identity with ``ops.coarse_score_wide`` where both
apply (one statement serves all three ops), its refusals, and the per-pair routing of
``coarse="any"`` (``gallery.coarse_routes``).

``STREAM_SHAPES`` and the synthetic case built from it also serve ``test_coarse_stream_gpu.py``."""
import pytest
import torch

from fpm import _lib, config, gallery, ops
from test_coarse_wide_cpu import SCALES, WIDE_SHAPES, synthetic_case
from test_shortlist_cpu import definition64

# (n0, n_g): single rows / columns at full length, both transposition cases, both sides of 256 and 512,
# nd = 300 dummy rows, small boxes (which "stream" must also take), the full box
STREAM_SHAPES = [(1, 1), (5, 2), (129, 129), (1, 600), (600, 1), (256, 257), (257, 257), (300, 600), (600, 300),
                 (385, 384), (513, 512), (520, 290), (600, 600)]

_CASES = {}


def stream_case(name):
    """``synthetic_case(name, STREAM_SHAPES)`` with the fp64 and fp32 host statements per probe, computed
    once per process and shared (read-only): (y, row_off, [(n0, yp, idx, coef, ref64, ref32)])."""
    if name not in _CASES:
        y, row_off, probes = synthetic_case(name, STREAM_SHAPES)
        out = []
        for n0, yp, idx, coef in probes:
            ref = ops.coarse_score_stream(y, row_off, idx, yp, coef, dtype=torch.float64)
            ref32 = ops.coarse_score_stream(y, row_off, idx, yp, coef)
            out.append((n0, yp, idx, coef, ref, ref32))
        _CASES[name] = (y, row_off, out)
    return _CASES[name]


def test_stream_bound_is_the_matchers():
    assert ops.COARSE_STREAM_NMAX == config.UNIV_SIZE == 600
    assert ops.COARSE_NMAX < ops.COARSE_WIDE_NMAX < ops.COARSE_STREAM_NMAX


@pytest.mark.parametrize("name", sorted(SCALES))
def test_stream_host_statement_is_the_definition(name):
    y, row_off, probes = stream_case(name)
    seen = set()
    for n0, yp, idx, coef, got, got32 in probes:
        assert got.dtype == torch.float64 and tuple(got.shape) == (idx.numel(),)
        for b, e in enumerate(idx.tolist()):
            yg = y[int(row_off[e]):int(row_off[e + 1])]
            ref = definition64(yp, coef[b], yg)
            assert abs(float(got[b]) - ref) <= 1e-12, (n0, yg.shape[0], float(got[b]), ref)
            seen.add((n0, int(yg.shape[0])))
        assert float(got[0]) == float(got[-1])                   # the entry listed twice
        assert got32.dtype == torch.float32
        assert float((got32.double() - got).abs().max()) < 1e-5
    assert set(STREAM_SHAPES) <= seen
    assert max(max(a, b) for a, b in seen) == ops.COARSE_STREAM_NMAX


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_stream_host_equals_wide_host_up_to_256(dtype):
    """All ops run the one host statement: the same bits on every box the wide op takes."""
    y, row_off, probes = synthetic_case("spread", WIDE_SHAPES)
    assert max(max(a, b) for a, b in WIDE_SHAPES) == ops.COARSE_WIDE_NMAX
    for n0, yp, idx, coef in probes:
        a = ops.coarse_score_wide(y, row_off, idx, yp, coef, dtype=dtype)
        b = ops.coarse_score_stream(y, row_off, idx, yp, coef, dtype=dtype)
        assert a.dtype == b.dtype == dtype
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), n0
        out = torch.empty(idx.numel(), dtype=dtype)
        assert ops.coarse_score_stream(y, row_off, idx, yp, coef, dtype=dtype, out=out) is out and torch.equal(out, a)


def test_stream_host_refusals():
    y = torch.zeros(1214, 768)
    row_off = torch.tensor([0, 3, 604, 1204, 1214], dtype=torch.int64)      # entries of 3, 601, 600, 10
    yp, coef = torch.zeros(4, 768), torch.zeros(2, 768)
    idx = torch.tensor([0, 2], dtype=torch.int32)
    ops.coarse_score_stream(y, row_off, idx, yp, coef, iters=1)               # 600 keypoints: taken
    ops.coarse_score_stream(y, row_off, idx[:1], torch.zeros(600, 768), coef[:1], iters=1)
    with pytest.raises(_lib.FpmError, match="COARSE_WIDE_NMAX"):              # ... and refused by the wide op
        ops.coarse_score_wide(y, row_off, idx, yp, coef)
    with pytest.raises(_lib.FpmError, match="coarse_score_stream: idx must be a int32"):
        ops.coarse_score_stream(y, row_off, idx.long(), yp, coef)
    with pytest.raises(_lib.FpmError, match="coarse_score_stream: idx must be a contiguous"):
        ops.coarse_score_stream(y, row_off, torch.stack([idx, idx], 1)[:, 0], yp, coef)
    with pytest.raises(_lib.FpmError, match=r"coarse_score_stream: idx value outside \[0, 4\)"):
        ops.coarse_score_stream(y, row_off, torch.tensor([0, 4], dtype=torch.int32), yp, coef)
    with pytest.raises(_lib.FpmError, match="n_g = 601.*COARSE_STREAM_NMAX = 600"):
        ops.coarse_score_stream(y, row_off, torch.tensor([0, 1], dtype=torch.int32), yp, coef)
    with pytest.raises(_lib.FpmError, match="probe of 601 keypoints.*COARSE_STREAM_NMAX = 600"):
        ops.coarse_score_stream(y, row_off, idx, torch.zeros(601, 768), coef)
    with pytest.raises(_lib.FpmError, match="coarse_score_stream coef"):
        ops.coarse_score_stream(y, row_off, idx, yp, torch.zeros(3, 768))
    with pytest.raises(_lib.FpmError, match="coarse_score_stream: yp must be contiguous fp32 rows"):
        ops.coarse_score_stream(y, row_off, idx, yp.double(), coef)
    with pytest.raises(_lib.FpmError, match="coarse_score_stream: yp must be contiguous fp32 rows"):
        ops.coarse_score_stream(y, row_off, idx, torch.zeros(768, 4).t(), coef)
    with pytest.raises(_lib.FpmError, match="coarse_score_stream: idx is on meta, y on cpu"):
        ops.coarse_score_stream(y, row_off, idx.to("meta"), yp, coef)
    with pytest.raises(_lib.FpmError, match="coarse_score_stream: iters >= 0 and tau > 0"):
        ops.coarse_score_stream(y, row_off, idx, yp, coef, tau=0.0)
    # the wide and fused ops' messages are what they were
    with pytest.raises(_lib.FpmError, match="coarse_score_wide: idx is on meta, y on cpu"):
        ops.coarse_score_wide(y, row_off, idx.to("meta"), yp, coef)
    with pytest.raises(_lib.FpmError, match="coarse_score_wide: a selected entry has n_g = 600; the coarse pass takes "
                                            "1 to COARSE_WIDE_NMAX = 256"):
        ops.coarse_score_wide(y, row_off, idx, yp, coef)
    with pytest.raises(_lib.FpmError, match="coarse_score_wide: a probe of 257 keypoints; the coarse pass takes 1 to "
                                            "COARSE_WIDE_NMAX = 256"):
        ops.coarse_score_wide(y, row_off, idx[:1], torch.zeros(257, 768), coef[:1])
    with pytest.raises(_lib.FpmError, match="coarse_score: a selected entry has n_g = 600; the coarse pass takes 1 to "
                                            "COARSE_NMAX = 128"):
        ops.coarse_score(y, row_off, idx, yp, coef)
    with pytest.raises(_lib.FpmError, match="coarse_score: a probe of 129 keypoints; the coarse pass takes 1 to "
                                            "COARSE_NMAX = 128"):
        ops.coarse_score(y, row_off, idx[:1], torch.zeros(129, 768), coef[:1])


def test_routes_per_pair():
    ng = torch.tensor([100, 128, 129, 256, 257, 600], dtype=torch.int32)
    assert gallery.COARSE_ROUTES == ("fused", "wide", "auto", "stream", "any")
    assert gallery.coarse_routes(120, ng, "any").tolist() == [0, 0, 1, 1, 2, 2]
    assert gallery.coarse_routes(200, ng, "any").tolist() == [1, 1, 1, 1, 2, 2]
    assert gallery.coarse_routes(300, ng, "any").tolist() == [2, 2, 2, 2, 2, 2]
    assert gallery.coarse_routes(120, ng).tolist() == [0, 0, 1, 1, 2, 2]             # "any" is the helper's default
    for n0 in (120, 200, 300):
        assert gallery.coarse_routes(n0, ng, "stream").tolist() == [2] * 6
    # the earlier routes are what they were
    assert gallery.coarse_routes(120, ng[:4], "auto").tolist() == [0, 0, 1, 1]
    assert gallery.coarse_routes(200, ng[:4], "auto").tolist() == [1, 1, 1, 1]
    assert gallery.coarse_routes(120, ng[:4], "wide").tolist() == [1, 1, 1, 1]
    assert gallery.coarse_routes(120, ng[:2], "fused").tolist() == [0, 0]
    for n0, sel in ((120, ng[:5]), (257, ng[:4])):
        for coarse in ("auto", "wide"):
            with pytest.raises(_lib.FpmError, match=r"a graph of 257 keypoints.*COARSE_WIDE_NMAX = 256 \(identify "
                                                    r"without a shortlist has no such bound\)"):
                gallery.coarse_routes(n0, sel, coarse)
    with pytest.raises(_lib.FpmError, match=r"a graph of 129 keypoints.*COARSE_NMAX = 128 \(identify"):
        gallery.coarse_routes(120, ng[:3], "fused")
    big = torch.tensor([100, 601], dtype=torch.int32)
    for coarse in ("stream", "any"):
        with pytest.raises(_lib.FpmError, match=r"a graph of 601 keypoints.*COARSE_STREAM_NMAX = 600 \(identify "
                                                r"without a shortlist has no such bound\)$"):
            gallery.coarse_routes(120, big, coarse)
        with pytest.raises(_lib.FpmError, match="a graph of 601 keypoints.*COARSE_STREAM_NMAX = 600"):
            gallery.coarse_routes(601, ng, coarse)
    with pytest.raises(_lib.FpmError, match=r"coarse must be one of \('fused', 'wide', 'auto', 'stream', 'any'\)"):
        gallery.coarse_routes(120, ng, "narrow")

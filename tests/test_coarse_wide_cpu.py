"""The wide coarse score (boxes of up to 256 keypoints), host side (no GPU): ``ops.coarse_score_wide``
on CPU tensors against the definition assembled from the oracle's pieces on shapes over 128, its
identity with ``ops.coarse_score`` where both apply (one statement serves both), and its refusals.

The synthetic case here (shapes, rows, coefficients) also serves ``test_coarse_wide_gpu.py``."""
import pytest
import torch

from fpm import _lib, ops
from test_shortlist_cpu import SHAPES, definition64

# (n0, n_g): single rows / columns, both transposition cases, one over the fused bound, both sides of
# the 64-, 128- and 192-row wave and fragment edges, the full box
WIDE_SHAPES = [(1, 1), (5, 2), (1, 129), (129, 1), (129, 129), (128, 129), (130, 256), (256, 130), (193, 192),
               (65, 250), (200, 145), (256, 256)]
PROBE_NS = sorted({a for a, _ in WIDE_SHAPES})
ENTRY_NS = sorted({b for _, b in WIDE_SHAPES})
SCALES = {"flat": 0.02, "spread": 0.22}          # the rows' standard deviation


def synthetic_case(name, shapes=WIDE_SHAPES):
    """Seeded N(0, 1) * s rows of 768 channels: one ragged index with an entry of every n_g of
    ``shapes`` and one probe per n0.  The probe's first min(n0, 200) rows are the largest entry's rows
    plus 0.1 s N(0, 1), so a dominant assignment exists.  Per probe the index list of the entries it
    meets in ``shapes`` (the first of them once more at the end) and coef = tanh(N(0, 1)) per listed
    entry.  -> (y, row_off, [(n0, yp, idx, coef)])."""
    s = SCALES[name]
    g = torch.Generator().manual_seed(1234 + len(name))
    entry_ns = sorted({b for _, b in shapes})
    rows = [torch.randn(n, 768, generator=g) * s for n in entry_ns]
    big = rows[-1]
    row_off = torch.tensor([0] + [sum(entry_ns[:i + 1]) for i in range(len(entry_ns))], dtype=torch.int64)
    probes = []
    for n0 in sorted({a for a, _ in shapes}):
        yp = torch.randn(n0, 768, generator=g) * s
        m = min(n0, 200, big.shape[0])
        yp[:m] = big[:m] + 0.1 * s * torch.randn(m, 768, generator=g)
        met = [entry_ns.index(b) for a, b in shapes if a == n0]
        idx = torch.tensor(met + met[:1], dtype=torch.int32)
        coef = torch.tanh(torch.randn(idx.numel(), 768, generator=g))
        coef[-1] = coef[0]
        probes.append((n0, yp.contiguous(), idx, coef.contiguous()))
    return torch.cat(rows).contiguous(), row_off, probes


@pytest.mark.parametrize("name", sorted(SCALES))
def test_wide_host_statement_is_the_definition(name):
    y, row_off, probes = synthetic_case(name)
    seen = set()
    for n0, yp, idx, coef in probes:
        got = ops.coarse_score_wide(y, row_off, idx, yp, coef, dtype=torch.float64)
        assert got.dtype == torch.float64 and tuple(got.shape) == (idx.numel(),)
        for b, e in enumerate(idx.tolist()):
            yg = y[int(row_off[e]):int(row_off[e + 1])]
            ref = definition64(yp, coef[b], yg)
            assert abs(float(got[b]) - ref) <= 1e-12, (n0, yg.shape[0], float(got[b]), ref)
            seen.add((n0, int(yg.shape[0])))
        assert float(got[0]) == float(got[-1])                   # the entry listed twice
        got32 = ops.coarse_score_wide(y, row_off, idx, yp, coef)
        assert got32.dtype == torch.float32
        assert float((got32.double() - got).abs().max()) < 1e-5
    assert set(WIDE_SHAPES) <= seen
    assert max(max(a, b) for a, b in seen) == ops.COARSE_WIDE_NMAX == 256


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_wide_host_equals_fused_host_up_to_128(dtype):
    """Both ops run the one host statement: the same bits on every box the fused op takes."""
    y, row_off, probes = synthetic_case("spread", SHAPES)
    assert max(max(a, b) for a, b in SHAPES) == ops.COARSE_NMAX
    for n0, yp, idx, coef in probes:
        a = ops.coarse_score(y, row_off, idx, yp, coef, dtype=dtype)
        b = ops.coarse_score_wide(y, row_off, idx, yp, coef, dtype=dtype)
        assert a.dtype == b.dtype == dtype
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), n0
        out = torch.empty(idx.numel(), dtype=dtype)
        assert ops.coarse_score_wide(y, row_off, idx, yp, coef, dtype=dtype, out=out) is out and torch.equal(out, a)


def test_wide_host_refusals():
    y = torch.zeros(400, 768)
    row_off = torch.tensor([0, 3, 260, 390, 400], dtype=torch.int64)       # entries of 3, 257, 130, 10
    yp, coef = torch.zeros(4, 768), torch.zeros(2, 768)
    idx = torch.tensor([0, 2], dtype=torch.int32)
    ops.coarse_score_wide(y, row_off, idx, yp, coef)                          # 130 keypoints: taken
    ops.coarse_score_wide(y, row_off, idx, torch.zeros(256, 768), coef)
    with pytest.raises(_lib.FpmError, match="COARSE_NMAX"):                   # ... and refused by the fused op
        ops.coarse_score(y, row_off, idx, yp, coef)
    with pytest.raises(_lib.FpmError, match="coarse_score_wide: idx must be a int32"):
        ops.coarse_score_wide(y, row_off, idx.long(), yp, coef)
    with pytest.raises(_lib.FpmError, match="coarse_score_wide: idx must be a contiguous"):
        ops.coarse_score_wide(y, row_off, torch.stack([idx, idx], 1)[:, 0], yp, coef)
    with pytest.raises(_lib.FpmError, match=r"coarse_score_wide: idx value outside \[0, 4\)"):
        ops.coarse_score_wide(y, row_off, torch.tensor([0, 4], dtype=torch.int32), yp, coef)
    with pytest.raises(_lib.FpmError, match="n_g = 257.*COARSE_WIDE_NMAX = 256"):
        ops.coarse_score_wide(y, row_off, torch.tensor([0, 1], dtype=torch.int32), yp, coef)
    with pytest.raises(_lib.FpmError, match="probe of 257 keypoints.*COARSE_WIDE_NMAX = 256"):
        ops.coarse_score_wide(y, row_off, idx, torch.zeros(257, 768), coef)
    with pytest.raises(_lib.FpmError, match="coarse_score_wide coef"):
        ops.coarse_score_wide(y, row_off, idx, yp, torch.zeros(3, 768))
    with pytest.raises(_lib.FpmError, match="coarse_score_wide: yp must be contiguous fp32 rows"):
        ops.coarse_score_wide(y, row_off, idx, yp.double(), coef)
    with pytest.raises(_lib.FpmError, match="coarse_score_wide: yp must be contiguous fp32 rows"):
        ops.coarse_score_wide(y, row_off, idx, torch.zeros(768, 4).t(), coef)
    with pytest.raises(_lib.FpmError, match="coarse_score_wide: idx is on meta, y on cpu"):
        ops.coarse_score_wide(y, row_off, idx.to("meta"), yp, coef)
    with pytest.raises(_lib.FpmError, match="coarse_score_wide: iters >= 0 and tau > 0"):
        ops.coarse_score_wide(y, row_off, idx, yp, coef, tau=0.0)
    # the fused op's messages are what they were
    with pytest.raises(_lib.FpmError, match="coarse_score: idx is on meta, y on cpu"):
        ops.coarse_score(y, row_off, idx.to("meta"), yp, coef)
    with pytest.raises(_lib.FpmError, match="coarse_score: a selected entry has n_g = 130; the coarse pass takes 1 to "
                                            "COARSE_NMAX = 128"):
        ops.coarse_score(y, row_off, idx, yp, coef)
    with pytest.raises(_lib.FpmError, match="coarse_score: a probe of 129 keypoints; the coarse pass takes 1 to "
                                            "COARSE_NMAX = 128"):
        ops.coarse_score(y, row_off, idx[:1], torch.zeros(129, 768), coef[:1])

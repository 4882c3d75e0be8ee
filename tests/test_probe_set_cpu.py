"""Probe sets, host side (no GPU): ``ops.coarse_pairs`` on CPU tensors against ``ops.coarse_score`` per
probe, its refusals (before any launch), ``gallery.probe_groups``, the per-pair ``gallery.coarse_routes``
and the probe-set refusals of ``match_pairs`` / ``coarse_scores_many`` / ``identify_many``."""
import types

import pytest
import torch

from fpm import _lib, gallery, ops
from test_compact_index_cpu import case, hand_index
from test_shortlist_cpu import ENTRY_NS, PROBE_NS, SHAPES, coefficients


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ------------------------------------------------------------------------------- the host statement
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_coarse_pairs_host_is_coarse_score_per_probe(dtype):
    """All probes of ``ragged_case`` stacked into one row store; the pair list is the concatenation of
    each probe's index list."""
    sd, y, row_off, wg, probes = case()
    yq = torch.cat([yp for yp, _ in probes])
    qrow_off = torch.tensor([0] + [sum(PROBE_NS[:i + 1]) for i in range(len(PROBE_NS))], dtype=torch.int64)
    idx = torch.tensor(list(range(len(ENTRY_NS))) + [2], dtype=torch.int32)      # one entry twice
    refs, coefs, seen = [], [], set()
    for q, (yp, wp) in enumerate(probes):
        coef = coefficients(wp, [wg[i] for i in idx.tolist()], sd)
        refs.append(ops.coarse_score(y, row_off, idx, yp, coef, dtype=dtype))
        coefs.append(coef)
        seen |= {(PROBE_NS[q], ENTRY_NS[g]) for g in idx.tolist()}
    assert set(SHAPES) <= seen
    gidx = idx.repeat(len(probes))
    qidx = torch.arange(len(probes), dtype=torch.int32).repeat_interleave(idx.numel())
    got = ops.coarse_pairs(y, row_off, gidx, yq, qrow_off, qidx, torch.cat(coefs), dtype=dtype)
    ref = torch.cat(refs)
    assert got.dtype == dtype and tuple(got.shape) == (gidx.numel(),)
    assert bool(torch.isfinite(got).all()) and torch.equal(_bits(got), _bits(ref))
    # the host statement has no size bound of its own, and the kernel's name changes nothing in it
    if dtype == torch.float32:
        again = ops.coarse_pairs(y, row_off, gidx, yq, qrow_off, qidx, torch.cat(coefs), kernel="stream")
        assert torch.equal(_bits(again), _bits(ref))


def test_coarse_pairs_refusals(monkeypatch):
    def trap(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", trap)
    # entries of 3, 129, 257, 601 and 8 keypoints; probes of 4, 129, 257 and 601
    ns, qs = (3, 129, 257, 601, 8), (4, 129, 257, 601)
    off = lambda v: torch.tensor([0] + [sum(v[:i + 1]) for i in range(len(v))], dtype=torch.int64)
    y, row_off = torch.zeros(sum(ns), 768), off(ns)
    yq, qrow_off = torch.zeros(sum(qs), 768), off(qs)
    coef = torch.zeros(2, 768)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    gidx, qidx = i32(0, 4), i32(0, 0)
    for kernel in ("fused", "wide", "stream"):
        assert tuple(ops.coarse_pairs(y, row_off, gidx, yq, qrow_off, qidx, coef, kernel=kernel).shape) == (2,)
    with pytest.raises(_lib.FpmError, match="qidx must be a int32"):
        ops.coarse_pairs(y, row_off, gidx, yq, qrow_off, qidx.long(), coef)
    with pytest.raises(_lib.FpmError, match="gidx must be a int32"):
        ops.coarse_pairs(y, row_off, gidx.long(), yq, qrow_off, qidx, coef)
    with pytest.raises(_lib.FpmError, match="qidx must be a contiguous"):
        ops.coarse_pairs(y, row_off, gidx, yq, qrow_off, torch.stack([qidx, qidx], 1)[:, 0], coef)
    with pytest.raises(_lib.FpmError, match="gidx must be a contiguous"):
        ops.coarse_pairs(y, row_off, torch.stack([gidx, gidx], 1)[:, 0], yq, qrow_off, qidx, coef)
    for bad in (i32(0, 4), i32(-1, 0)):
        with pytest.raises(_lib.FpmError, match=r"qidx value outside \[0, 4\)"):
            ops.coarse_pairs(y, row_off, gidx, yq, qrow_off, bad, coef)
    with pytest.raises(_lib.FpmError, match=r"gidx value outside \[0, 5\)"):
        ops.coarse_pairs(y, row_off, i32(0, 5), yq, qrow_off, qidx, coef)
    with pytest.raises(_lib.FpmError, match="gidx names 2 pairs, qidx 3"):
        ops.coarse_pairs(y, row_off, gidx, yq, qrow_off, i32(0, 0, 0), coef)
    # a probe or an entry over the kernel's bound, for each kernel: entry / probe number 1, 2, 3
    for k, (kernel, bound) in enumerate((("fused", "COARSE_NMAX"), ("wide", "COARSE_WIDE_NMAX"),
                                         ("stream", "COARSE_STREAM_NMAX"))):
        with pytest.raises(_lib.FpmError, match="a selected entry of %d keypoints.*%s = " % (ns[k + 1], bound)):
            ops.coarse_pairs(y, row_off, i32(0, k + 1), yq, qrow_off, qidx, coef, kernel=kernel)
        with pytest.raises(_lib.FpmError, match="a probe of %d keypoints.*%s = " % (qs[k + 1], bound)):
            ops.coarse_pairs(y, row_off, gidx, yq, qrow_off, i32(0, k + 1), coef, kernel=kernel)
        if k:                                                    # ... which the next kernel up takes
            ops.coarse_pairs(y, row_off, i32(0, k), yq, qrow_off, i32(0, k), coef, kernel=kernel)
    for bad in (torch.zeros(3, 768), torch.zeros(2, 767)):
        with pytest.raises(_lib.FpmError, match="coef"):
            ops.coarse_pairs(y, row_off, gidx, yq, qrow_off, qidx, bad)
    with pytest.raises(_lib.FpmError, match="kernel must be one of"):
        ops.coarse_pairs(y, row_off, gidx, yq, qrow_off, qidx, coef, kernel="auto")
    with pytest.raises(_lib.FpmError, match="yq must be contiguous fp32 rows"):
        ops.coarse_pairs(y, row_off, gidx, yq.to(torch.bfloat16), qrow_off, qidx, coef)
    with pytest.raises(_lib.FpmError, match="qrow_off must rise from 0"):
        ops.coarse_pairs(y, row_off, gidx, yq[:-1], qrow_off, qidx, coef)


# ------------------------------------------------------------------------------------- probe_groups
def test_probe_groups():
    n = [50, 20, 40, 20, 30]
    # stable ascending order of n: probes 1, 3 (both 20, in index order), 4, 2, 0; 8 pairs each
    assert gallery.probe_groups(n, 8, 16) == [[1, 3], [4, 2], [0]]
    assert gallery.probe_groups(n, 8, 17) == [[1, 3], [4, 2], [0]]
    assert gallery.probe_groups(n, 8, 24) == [[1, 3, 4], [2, 0]]
    assert gallery.probe_groups(n, 8, 1000) == [[1, 3, 4, 2, 0]]
    assert gallery.probe_groups(torch.tensor(n, dtype=torch.int32), 8, 8) == [[1], [3], [4], [2], [0]]
    # a probe whose own pairs exceed group_pairs is a group alone
    assert gallery.probe_groups(n, 8, 5) == [[1], [3], [4], [2], [0]]
    assert gallery.probe_groups(n, [3, 3, 9, 3, 3], 6) == [[1, 3], [4], [2], [0]]
    # every probe in exactly one group, whatever the sizes
    g = torch.Generator().manual_seed(1)
    for cap in (1, 7, 64, 10 ** 6):
        nn = torch.randint(1, 600, (37,), generator=g)
        per = torch.randint(1, 40, (37,), generator=g)
        groups = gallery.probe_groups(nn, per, cap)
        flat = [i for grp in groups for i in grp]
        assert sorted(flat) == list(range(37))
        assert flat == torch.argsort(nn, stable=True).tolist()
        for grp in groups:
            assert len(grp) == 1 or int(per[grp].sum()) <= cap
        for a, b in zip(groups, groups[1:]):                     # packed: the next probe did not fit
            assert int(per[a].sum()) + int(per[b[0]]) > cap
    assert gallery.probe_groups([], 8, 16) == []
    with pytest.raises(_lib.FpmError, match="one count or one per probe"):
        gallery.probe_groups(n, [8, 8], 16)
    with pytest.raises(_lib.FpmError, match="at least 1"):
        gallery.probe_groups(n, 8, 0)


# ----------------------------------------------------------------------------------- per-pair routes
def test_per_pair_routes():
    nq = torch.tensor([120, 129, 257])
    ng = torch.tensor([100, 128, 129, 256, 257, 600])
    q, g = nq.repeat_interleave(ng.numel()), ng.repeat(nq.numel())
    side = torch.maximum(q, g)
    rt = gallery.coarse_routes(q, g, "any")
    assert rt.dtype == torch.int64 and rt.tolist() == [0 if s <= 128 else 1 if s <= 256 else 2 for s in side.tolist()]
    assert set(rt.tolist()) == {0, 1, 2}
    # the per-pair form agrees with the one-probe form, probe by probe
    for i, n0 in enumerate(nq.tolist()):
        assert torch.equal(rt[i * 6:(i + 1) * 6], gallery.coarse_routes(n0, ng, "any"))
    ok = side <= 256
    rt = gallery.coarse_routes(q[ok], g[ok], "auto")
    assert rt.tolist() == [0 if s <= 128 else 1 for s in side[ok].tolist()]
    with pytest.raises(_lib.FpmError, match="COARSE_WIDE_NMAX"):
        gallery.coarse_routes(q, g, "auto")
    with pytest.raises(_lib.FpmError, match="COARSE_WIDE_NMAX"):
        gallery.coarse_routes(torch.tensor([257, 4]), torch.tensor([4, 4]), "auto")       # the probe alone is over
    # the fixed routes: every pair on that kernel, refused over its bound on either side
    small = side <= 128
    assert gallery.coarse_routes(q[small], g[small], "fused").tolist() == [0] * int(small.sum())
    assert gallery.coarse_routes(q[ok], g[ok], "wide").tolist() == [1] * int(ok.sum())
    assert gallery.coarse_routes(q, g, "stream").tolist() == [2] * q.numel()
    for coarse, bound in (("fused", "COARSE_NMAX"), ("wide", "COARSE_WIDE_NMAX")):
        with pytest.raises(_lib.FpmError, match=bound + " ="):
            gallery.coarse_routes(q, g, coarse)
    with pytest.raises(_lib.FpmError, match="COARSE_NMAX ="):
        gallery.coarse_routes(torch.tensor([129, 4]), torch.tensor([4, 4]), "fused")
    with pytest.raises(_lib.FpmError, match="COARSE_STREAM_NMAX"):
        gallery.coarse_routes(torch.tensor([601, 4]), torch.tensor([4, 4]), "stream")
    with pytest.raises(_lib.FpmError, match="one count or one per pair"):
        gallery.coarse_routes(torch.tensor([4, 4, 4]), torch.tensor([4, 4]), "any")


# ------------------------------------------------------------------------------- probe-set refusals
def _calls(net, probes, index, **kw):
    return (lambda: gallery.match_pairs(net, probes, index, [(0, 0)]),
            lambda: gallery.coarse_scores_many(net, probes, index),
            lambda: gallery.identify_many(net, probes, index, **kw))


def test_probe_set_refusals():
    net = types.SimpleNamespace(training=False, use_graphs=False)        # refused before the net is asked anything
    index = hand_index("f32")
    for call in _calls(net, hand_index("bf16+host"), index):
        with pytest.raises(_lib.FpmError, match="probe set's layout is 'bf16\\+host'"):
            call()
    other = hand_index("f32+bf16")
    other.sc_mode = "bf16"
    for call in _calls(net, other, index):
        with pytest.raises(_lib.FpmError, match="sc_mode 'bf16', the gallery with 'f32'"):
            call()
    other = hand_index("f32")
    other.weights_id = "ffff0000"
    for call in _calls(net, other, index):
        with pytest.raises(_lib.FpmError, match="different SplineConv weights"):
            call()
    for call in _calls(net, {"n": 3}, index):
        with pytest.raises(_lib.FpmError, match="probes must be a probe set"):
            call()
    with pytest.raises(_lib.FpmError, match="exclude_self"):
        gallery.identify_many(net, hand_index("f32"), index, shortlist=2, exclude_self=True)
    # the refusals of identify apply: training mode, HIP-graph replay
    for flags, msg in ((dict(training=True, use_graphs=False), "inference only"),
                       (dict(training=False, use_graphs=True), "use_graphs")):
        for call in _calls(types.SimpleNamespace(**flags), hand_index("f32+bf16"), index):
            with pytest.raises(_lib.FpmError, match=msg):
                call()

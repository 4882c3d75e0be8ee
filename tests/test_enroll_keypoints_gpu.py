"""Enrolment and probes from keypoints and images on the GPU: the ragged pack kernel against its torch
statement and ``ops.cast_bf16`` (bit for bit), ``Net.enroll_keypoints`` against ``Net.enroll`` on the same
graphs as host dicts (every field of the index), device probes (``Net.probe_graphs``) through ``identify`` /
``coarse_scores`` against the uncached forward and the numpy probe, a keypoint-enrolled probe set, and the
image path on captured backbone features."""
import numpy as np
import pytest
import torch

import fpm
from fpm import _lib, graphs, ops, params
from fpm.batch import DeviceBatch
from test_enroll_keypoints_cpu import PACK_NMAX, pack_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
OUT_KEYS = ("s", "ss", "ds_mat", "perm_mat", "k_prob", "cls_prob")
FIELDS = ("y", "y16", "row_off", "n", "src", "dst", "pseudo", "edge_off", "w", "P", "sc_mode", "weights_id")
LAYOUTS = ("f32", "f32+bf16", "bf16+host")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_index(a, b):
    for k in FIELDS:
        u, v = getattr(a, k), getattr(b, k)
        if isinstance(u, torch.Tensor):
            assert u.dtype == v.dtype and u.device == v.device and torch.equal(u, v), k
        else:
            assert u == v, k
    assert a.layout == b.layout and a.G == b.G


# --------------------------------------------------------------------------------------- rows_pack
@pytest.mark.parametrize("which", ["out32", "out16", "both"])
def test_rows_pack_bits(which):
    """Band edges, an empty and a full graph, specials in the rows, NaN in the padding and in the outputs:
    out32 is the torch statement, out16 is ``ops.cast_bf16`` of it, nothing else is written."""
    src, n, off, want = pack_case()
    total = int(off[-1])
    want16 = ops.cast_bf16(want.to(DEV))
    o32 = torch.full((total + 3, 768), float("nan"), device=DEV) if which != "out16" else None
    o16 = torch.full((total + 3, 768), float("nan"), device=DEV, dtype=torch.bfloat16) if which != "out32" else None
    ops.rows_pack(src.to(DEV), n.to(DEV), PACK_NMAX, off.to(DEV), out32=o32, out16=o16)
    torch.cuda.synchronize()
    if o32 is not None:
        assert torch.equal(o32[:total].cpu(), want) and torch.equal(_bits(o32[:total].cpu()), _bits(want))
        assert bool(torch.isnan(o32[total:]).all())
    if o16 is not None:
        assert torch.equal(_bits(o16[:total]), _bits(want16))
        assert torch.equal(_bits(o16[:total].cpu()), _bits(want.to(torch.bfloat16)))
        assert bool(torch.isnan(o16[total:]).all())


# ------------------------------------------------------------------------------ keypoint galleries
@pytest.fixture(scope="module")
def sd():
    return params.init_params(7)


def _net(sd, dtype):
    net = fpm.Net(regression=True, backbone=False, dtype=dtype)
    net.load_state_dict(sd)
    return net


CASES = {
    # as test_gallery_gpu.CASES: (net dtype, probe keypoints, gallery keypoints, sc_mode)
    "f32ops-f32": ("f32", 48, [48, 40, 45, 48, 37, 48], "f32"),
    "f32ops-bf16": ("bf16", 48, [48, 40, 45, 48, 37, 48], "f32"),
    "bf16ops": ("bf16", 72, [72, 65, 70, 51], None),
}


def _keypoint_set(ns, seed):
    """Random distinct keypoints (zero padding), node and global features of len(ns) graphs (host)."""
    g = torch.Generator().manual_seed(seed)
    G, nmax = len(ns), max(ns)
    n = torch.tensor(ns, dtype=torch.int32)
    keep = (torch.arange(nmax)[None, :] < n.view(-1, 1))[..., None]
    P = torch.rand(G, nmax, 2, generator=g) * torch.tensor([320.0, 240.0]) * keep
    x = torch.randn(G, nmax, 768, generator=g) * keep
    w = torch.rand(G, 512, generator=g)
    return P, n, x, w


def _export(P, n, x, w):
    """The graphs of a keypoint set built once on the device, as host graph dicts."""
    nmax = int(P.shape[1])
    gb = graphs.build_graph_batch(P.to(DEV), n)
    eo = gb.edge_off_host.tolist()
    src, dst, ps = (gb.src % nmax).cpu().numpy(), (gb.dst % nmax).cpu().numpy(), gb.pseudo.cpu().numpy()
    return [dict(n=int(k), x=x[g, :k].numpy(), w=w[g].numpy(), P=P[g, :k].numpy(),
                 edge_index=np.stack([src[eo[g]:eo[g + 1]], dst[eo[g]:eo[g + 1]]]), pseudo=ps[eo[g]:eo[g + 1]])
            for g, k in enumerate(n.tolist())]


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request, sd):
    dtype, n_probe, ns, sc_mode = CASES[request.param]
    net = _net(sd, dtype)
    gal = _keypoint_set(ns, 11)
    prb = _keypoint_set([n_probe], 12)
    dicts, pdict = _export(*gal), _export(*prb)[0]
    index = {lay: net.enroll_keypoints(*[t.to(DEV) for t in gal], sc_mode=sc_mode, batch=4, layout=lay)
             for lay in LAYOUTS}
    return dict(net=net, gal=gal, prb=prb, dicts=dicts, pdict=pdict, index=index, sc_mode=sc_mode)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_index_equals_host_dict_enrolment(case, layout):
    """batch=4 over 6 / 4 graphs: two sub-batches with different trims (or one trimmed to its own largest)."""
    net = case["net"]
    ref = net.enroll(case["dicts"], DEV, sc_mode=case["sc_mode"], batch=4, layout=layout)
    _same_index(ref, case["index"][layout])
    assert case["index"][layout].y.is_cuda == (layout != "bf16+host")
    # host inputs (arrays and the flat feature layout), device named: the same index
    P, n, x, w = case["gal"]
    host = net.enroll_keypoints(P.numpy(), n.tolist(), x.view(-1, 768), w.numpy(), device=DEV,
                                sc_mode=case["sc_mode"], batch=4, layout=layout)
    _same_index(ref, host)


def _probe_ref(net, prb, gal, sel):
    """The uncached forward of the probe repeated x the gallery entries ``sel``, graphs built on the device."""
    Pp, npr, xp, wp = prb
    Pg, ng, xg, wg = (t[sel] for t in gal)
    B, n0 = len(sel), int(Pp.shape[1])
    assert int(ng.max()) == Pg.shape[1]                 # a full-size entry: the padded boxes coincide
    bt = DeviceBatch.from_keypoints([Pp.expand(B, -1, -1).contiguous().to(DEV), Pg.to(DEV)], [npr.expand(B), ng],
                                    [xp.expand(B, -1, -1).reshape(B * n0, 768).contiguous().to(DEV),
                                     xg.reshape(-1, 768).contiguous().to(DEV)],
                                    [wp.expand(B, -1).contiguous().to(DEV), wg.to(DEV)], DEV)
    return net.run(bt, chunks=2)


def test_device_probe_identify_equals_uncached(case):
    net, index = case["net"], case["index"]["f32"]
    probe = net.probe_graphs(*[t.to(DEV) for t in case["prb"][:2]], x=case["prb"][2].to(DEV), w=case["prb"][3].to(DEV))
    assert len(probe) == 1 and probe[0]["n"] == case["prb"][0].shape[1]
    probe = probe[0]
    assert all(probe[k].is_cuda for k in ("x", "w", "edge_index", "pseudo", "P"))
    assert probe["edge_index"].dtype == torch.int32 and probe["edge_index"].shape[0] == 2
    for sel in (list(range(index.G)), [3, 0, 2]):
        ref = _probe_ref(net, case["prb"], case["gal"], sel)
        res = net.identify(probe, index, topk=3, chunks=2, select=sel)
        for k in OUT_KEYS:
            assert torch.equal(res[k], ref[k]), (k, sel)
        assert res["top_idx"].numel() == 3 and set(res["top_idx"].tolist()) <= set(sel)


def test_device_probe_equals_numpy_probe(case):
    net, idx = case["net"], case["index"]
    probe = net.probe_graphs(*case["prb"], device=DEV)[0]      # host inputs, staged on the device
    pd = case["pdict"]
    for k in ("x", "w", "edge_index", "pseudo", "P"):
        assert np.array_equal(probe[k].cpu().numpy(), pd[k]), k
    a = net.coarse_scores(probe, idx["f32"])
    b = net.coarse_scores(pd, idx["f32"])
    assert torch.equal(_bits(a), _bits(b))
    ra = net.identify(probe, idx["f32"], shortlist=3, topk=3, chunks=2)
    rb = net.identify(pd, idx["f32"], shortlist=3, topk=3, chunks=2)
    rc = net.identify(probe, idx["bf16+host"], shortlist=3, topk=3, chunks=2)
    for k in OUT_KEYS + ("top_idx", "top_score", "short_idx", "coarse_score", "coarse_all"):
        assert torch.equal(ra[k], rb[k]), k
        assert torch.equal(ra[k], rc[k]), k


def test_keypoint_probe_set(case):
    """A second keypoint-enrolled index as the probe set of identify_many: the host-dict-enrolled set's rows."""
    net, index = case["net"], case["index"]["f32"]
    nmax = int(case["gal"][0].shape[1])
    pk = _keypoint_set([nmax - 8, nmax, nmax - 15], 13)
    pset_k = net.enroll_keypoints(*pk, device=DEV, sc_mode=case["sc_mode"], batch=2)
    pset_d = net.enroll(_export(*pk), DEV, sc_mode=case["sc_mode"], batch=2)
    _same_index(pset_d, pset_k)
    ra = net.identify_many(pset_k, index, shortlist=3, topk=3)
    rb = net.identify_many(pset_d, index, shortlist=3, topk=3)
    assert len(ra) == len(rb) == 3
    for a, b in zip(ra, rb):
        for k in OUT_KEYS + ("top_idx", "top_score", "short_idx", "coarse_score", "coarse_all"):
            assert torch.equal(a[k], b[k]), k


def test_refusals(sd):
    net = _net(sd, "f32")
    P, n, x, w = (t.to(DEV) for t in _keypoint_set([9, 7], 14))
    net.train()
    try:
        with pytest.raises(_lib.FpmError, match="enroll_keypoints: inference only"):
            net.enroll_keypoints(P, n, x, w)
    finally:
        net.eval()
    for bad in ([9, 10], [0, 7]):
        with pytest.raises(_lib.FpmError, match=r"counts must lie in \[1, nmax = 9\]"):
            net.enroll_keypoints(P, torch.tensor(bad, device=DEV), x, w)
        with pytest.raises(_lib.FpmError, match=r"counts must lie in \[1, nmax = 9\]"):
            net.probe_graphs(P, bad, x=x, w=w)
    with pytest.raises(NotImplementedError, match="image input needs the backbone"):
        net.enroll_images(torch.zeros(2, 3, 32, 32, device=DEV), P, n)


# ------------------------------------------------------------------------------------------ images
def test_enroll_images_on_captured_features():
    """MIOpen's features are not reproducible call to call, so every comparison is on the features the call
    under test computed, captured by a spy on ``net.image_features``."""
    net = fpm.Net(regression=True, backbone=True)
    net.load_state_dict({**net.state_dict(), **params.init_params(5)})
    g = torch.Generator().manual_seed(4)
    G, nmax = 3, 32
    imgs = torch.rand(G, 3, 120, 160, generator=g)
    P, n, _, _ = _keypoint_set([32, 27, 22], 15)
    seen = []
    image_features = net.image_features

    def spy(images, Ps, ns, *a, **kw):
        out = image_features(images, Ps, ns, *a, **kw)
        seen.append((int(images[0].shape[0]), out))
        return out

    net.image_features = spy
    try:
        one = net.enroll_images(imgs, P, n, device=DEV, sc_mode="f32")
        assert [s[0] for s in seen] == [3]
        xs, gs = seen[0][1]
        x, w = xs[0].view(G, nmax, 768), gs[0]
        _same_index(net.enroll_keypoints(P, n, x, w, device=DEV, sc_mode="f32"), one)
        del seen[:]
        two = net.enroll_images(imgs.to(DEV), P.to(DEV), n, sc_mode="f32", batch=2, layout="f32+bf16")
        assert [s[0] for s in seen] == [2, 1]
        assert two.G == 3 and two.n.tolist() == [32, 27, 22] and two.row_off_host.tolist() == [0, 32, 59, 81]
        assert tuple(two.y.shape) == (81, 768) and tuple(two.y16.shape) == (81, 768)
        x2 = torch.cat([s[1][0][0].view(-1, nmax, 768) for s in seen])
        w2 = torch.cat([s[1][1][0] for s in seen])
        _same_index(net.enroll_keypoints(P, n, x2, w2, device=DEV, sc_mode="f32", batch=2, layout="f32+bf16"), two)
        del seen[:]
        probe = net.probe_graphs(P[:1], n[:1], images=imgs[:1], device=DEV)
        assert [s[0] for s in seen] == [1] and len(probe) == 1
        xs, gs = seen[0][1]
        again = net.probe_graphs(P[:1], n[:1], x=xs[0], w=gs[0], device=DEV)
    finally:
        net.image_features = image_features
    ra = net.identify(probe[0], one, topk=3)
    rb = net.identify(again[0], one, topk=3)
    for k in OUT_KEYS + ("top_idx", "top_score"):
        assert torch.equal(ra[k], rb[k]), k
    assert sorted(ra["top_idx"].tolist()) == [0, 1, 2]
    assert bool(torch.isfinite(ra["top_score"]).all())

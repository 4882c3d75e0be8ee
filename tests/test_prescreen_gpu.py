"""Prescreen of a 1:N identification on the GPU: ``ops.rows_pool`` and ``ops.rank_keep`` against their host
statements (bit for bit), ``ops.desc_score`` against float64 and its composition independence, the descriptors of
a ``GalleryIndex`` through every operation that carries them, ``Net.identify`` / ``identify_many(prescreen=K)``
against the selected queries (bit for bit), the refusals and the C-ABI.

Gate of the score test (the convention of ``test_shortlist_gpu.py``): ``ref`` is the host statement of the score
(``ops.desc_score`` on CPU tensors) in float64 on the same bf16 operands, ``ref32`` the same in float32,
``err32 = max |ref32 - ref|`` over the case.  The device must stay within ``max(8 ulp32(max |ref|), 8 err32)``.

MEASURED on an MI355X (the ``MEASURE`` lines): desc_score err 4.93e-08, err32 7.39e-07 (ratio 0.067), gate 5.91e-06,
scores -0.134 .. 1.  Planted gallery, probes 0 / 1 / 2: mate 0.953046 / 0.936893 / 0.936225, runner-up 0.085319 /
0.102355 / 0.082517, gap between the 8th and 9th score 1.64e-3 / 2.48e-3 / 4.05e-3, score gate 3.3e-6 .. 4.3e-6.
"""
import ctypes

import numpy as np
import pytest
import torch

from fpm import _lib, gallery, ops
from fpm.gallery import GalleryIndex
from fpm.sharded_gallery import ShardedGallery
from test_enroll_keypoints_gpu import _export
from test_prescreen_cpu import KEEP_SHAPES, POOL_NS, keep_scores, pool_case
from test_shortlist_cpu import state_dicts
from test_shortlist_gpu import MATES, OUT_KEYS, _net, planted

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# --------------------------------------------------------------------------------------------- pool
def test_rows_pool_device_equals_host():
    y, off = pool_case()
    ref = ops.rows_pool(y, off)
    y_d, off_d = y.to(DEV), off.to(DEV)
    full = ops.rows_pool(y_d, off_d, row_off_host=off)
    assert full.dtype == torch.bfloat16 and tuple(full.shape) == (len(POOL_NS), 768) and full.device == DEV
    assert torch.equal(_bits(full.cpu()), _bits(ref))
    assert not bool(_bits(full[-1]).any())
    for e in range(len(POOL_NS)):
        one = ops.rows_pool(y_d, off_d, e, e + 1, row_off_host=off)
        assert torch.equal(_bits(one.cpu()), _bits(ref[e:e + 1])), e
    out = torch.full((3, 768), 7.0, device=DEV, dtype=torch.bfloat16)
    assert ops.rows_pool(y_d, off_d, 2, 5, out=out) is out
    assert torch.equal(_bits(out.cpu()), _bits(ref[2:5]))
    bad = y.clone()
    bad[0, 5], bad[1, 9] = float("inf"), float("nan")
    assert torch.equal(_bits(ops.rows_pool(bad.to(DEV), off_d, row_off_host=off).cpu()), _bits(ops.rows_pool(bad, off)))


# -------------------------------------------------------------------------------------------- score
def _unit_desc(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, 768, generator=g), dim=1).to(torch.bfloat16).contiguous()


@pytest.fixture(scope="module")
def descs():
    dq, dg = _unit_desc(17, 5), _unit_desc(1000, 6)
    dg[11] = dq[3]                                               # one score near 1
    return dq, dg, ops.desc_score(dq, dg, dtype=torch.float64), ops.desc_score(dq, dg).double()


def test_desc_score_vs_float64(descs):
    dq, dg, ref, ref32 = descs
    dq_d, dg_d = dq.to(DEV), dg.to(DEV)
    err = 0.0
    for Q in (1, 5, 16, 17):
        for G in (1, 255, 256, 257, 1000):
            out = ops.desc_score(dq_d[:Q], dg_d[:G])
            assert out.dtype == torch.float32 and tuple(out.shape) == (Q, G)
            assert bool(torch.isfinite(out).all())
            err = max(err, float((out.cpu().double() - ref[:Q, :G]).abs().max()))
    err32 = float((ref32 - ref).abs().max())
    top = float(ref.abs().max())
    ulp = 2.0 ** (np.floor(np.log2(top)) - 23)
    gate = max(8 * ulp, 8 * err32)
    print("MEASURE desc_score err=%.3g err32=%.3g ratio=%.3g gate=%.3g scores=[%.3g, %.3g]"
          % (err, err32, err / err32, gate, float(ref.min()), float(ref.max())))
    assert err <= gate, "desc_score: device error %.3g over the gate %.3g (err32 %.3g)" % (err, gate, err32)


def test_desc_score_composition(descs):
    dq, dg, _, _ = descs
    dq_d, dg_d = dq.to(DEV), dg.to(DEV)
    full = ops.desc_score(dq_d, dg_d)
    alone = ops.desc_score(dq_d[3:4].contiguous(), dg_d)
    assert torch.equal(_bits(alone[0]), _bits(full[3]))                       # probe 3 alone / among 17
    seven = torch.tensor([7], dtype=torch.int32)
    one = ops.desc_score(dq_d, dg_d, seven.to(DEV), idx_host=seven)
    assert torch.equal(_bits(one[:, 0]), _bits(full[:, 7]))                   # entry 7 alone / in the full launch
    perm = torch.randperm(1000, generator=torch.Generator().manual_seed(9)).to(torch.int32)
    perm = torch.cat([perm[:500], perm[20:21], perm[500:]])                   # one entry twice
    mixed = ops.desc_score(dq_d, dg_d, perm.to(DEV), idx_host=perm)
    assert torch.equal(_bits(mixed), _bits(full[:, perm.long().to(DEV)]))
    # an idx outside [0, G): refused with a host copy, NaN from the kernel without one
    wild = torch.tensor([5, 1000, -1, 6], dtype=torch.int32)
    with pytest.raises(_lib.FpmError, match="outside"):
        ops.desc_score(dq_d, dg_d, wild.to(DEV), idx_host=wild)
    out = ops.desc_score(dq_d, dg_d, wild.to(DEV))
    assert bool(torch.isnan(out[:, 1:3]).all()) and torch.equal(_bits(out[:, [0, 3]]), _bits(full[:, [5, 6]]))


# --------------------------------------------------------------------------------------------- keep
@pytest.mark.parametrize("P,G,k", KEEP_SHAPES)
def test_rank_keep_device_equals_host(P, G, k):
    s = keep_scores(P, G, 31 * G + k)
    ref = ops.rank_keep(s, k)
    keep = ops.rank_keep(s.to(DEV), k)
    assert keep.dtype == torch.int32 and tuple(keep.shape) == (P, k) and keep.device == DEV
    assert torch.equal(keep.cpu(), ref)
    assert int(keep.min()) >= 0 and int(keep.max()) < G and bool((keep[:, 1:] > keep[:, :-1]).all())
    wide = torch.zeros(P, G + 9)                       # a strided view (row stride > G)
    wide[:, 4:4 + G] = s
    assert torch.equal(ops.rank_keep(wide.to(DEV)[:, 4:4 + G], k).cpu(), ref)


# -------------------------------------------------------------------------------------------- index
def _fresh(index):
    """The descriptors of an index's entries pooled afresh from its fp32 rows."""
    return ops.rows_pool(index.y.to(DEV).contiguous(), index.row_off, row_off_host=index.row_off_host)


def _same_desc(index, want=None):
    assert index.desc is not None and index.desc.dtype == torch.bfloat16 and index.desc.device == DEV
    assert tuple(index.desc.shape) == (index.G, 768)
    assert torch.equal(_bits(index.desc), _bits(_fresh(index) if want is None else want))


@pytest.fixture(scope="module")
def sd():
    return state_dicts()["spread"]


@pytest.fixture(scope="module")
def keypoint_gallery():
    """planted()'s 40 entries as padded keypoint arrays, and the same graphs (built once on the device) as host
    dicts: the two enrolment routes then see the same graphs."""
    gal, _ = planted()
    G, nmax = len(gal), max(g["n"] for g in gal)
    n = torch.tensor([g["n"] for g in gal], dtype=torch.int32)
    P, x = torch.zeros(G, nmax, 2), torch.zeros(G, nmax, 768)
    for i, g in enumerate(gal):
        P[i, :g["n"]], x[i, :g["n"]] = torch.from_numpy(g["P"]), torch.from_numpy(g["x"])
    w = torch.from_numpy(np.stack([g["w"] for g in gal]))
    return (P, n, x, w), _export(P, n, x, w)


@pytest.mark.parametrize("layout", ["f32", "fp8+host"])
def test_index_descriptors(layout, sd, keypoint_gallery, tmp_path):
    arrays, dicts = keypoint_gallery
    net = _net(sd)
    G = len(dicts)
    a = net.enroll(dicts, DEV, batch=16, layout=layout, descriptors=True)
    b = net.enroll_keypoints(*[t.to(DEV) for t in arrays], batch=16, layout=layout, descriptors=True)
    c = net.enroll(dicts, DEV, batch=16, layout=layout)
    assert c.desc is None and c.add_descriptors() is c
    d = net.enroll(dicts, DEV, batch=16, layout=layout).add_descriptors(chunk=100)      # several uploads on "+host"
    _same_desc(a)
    for other in (b, c, d):
        _same_desc(other, a.desc)
    assert bool(_bits(a.desc).any(1).all())
    assert a.nbytes() == net.enroll(dicts, DEV, batch=16, layout=layout).nbytes() + G * 1536
    # save / load: a new format number with descriptors, the old one without
    path = str(tmp_path / "index.pt")
    a.save(path)
    assert torch.load(path, weights_only=True)["format"] == gallery.FORMAT_DESC
    _same_desc(GalleryIndex.load(path, DEV), a.desc)
    roomy = GalleryIndex.load(path, DEV, capacity=(G + 4, int(a.y.shape[0]) + 200))
    _same_desc(roomy, a.desc)
    plain = net.enroll(dicts, DEV, batch=16, layout=layout)
    plain.save(path)
    assert torch.load(path, weights_only=True)["format"] == (gallery.FORMAT_FP8 if layout == "fp8+host" else gallery.FORMAT)
    back = GalleryIndex.load(path, DEV)
    assert back.desc is None and torch.equal(back.y.cpu(), plain.y.cpu())
    # reserve + enroll_into: the appended entries are pooled; a failed append leaves desc as it was
    extra = dicts[5:8]
    grown = a.reserve(G + 4, int(a.y.shape[0]) + 200)
    _same_desc(grown, a.desc)
    new = net.enroll_into(grown, extra, batch=2)
    assert new.tolist() == [G, G + 1, G + 2]
    _same_desc(grown)
    assert torch.equal(_bits(grown.desc[:G]), _bits(a.desc)) and torch.equal(_bits(grown.desc[G:]), _bits(a.desc[5:8]))
    tight = a.reserve(G + 4, int(a.y.shape[0]) + 200, edges=int(a.src.numel()) + 1)
    with pytest.raises(_lib.FpmError, match="edges"):
        net.enroll_into(tight, extra, batch=2)
    assert tight.G == G
    _same_desc(tight, a.desc)
    with pytest.raises(_lib.FpmError, match="add_descriptors"):
        net.enroll_into(plain.reserve(G + 4, int(a.y.shape[0]) + 200), extra, descriptors=True)
    # remove + compact, slice
    live = torch.tensor([e for e in range(G) if e not in (3, 7)])
    grown.remove([3, 7])
    _same_desc(grown)
    grown.compact()
    assert grown.G == G + 1
    _same_desc(grown)
    assert torch.equal(_bits(grown.desc[:G - 2]), _bits(a.desc[live.to(DEV)]))
    ent = torch.tensor([0, 4, 5, 17, 39])
    part = a.slice(ent)
    _same_desc(part)
    assert torch.equal(_bits(part.desc), _bits(a.desc[ent.to(DEV)]))
    shards = ShardedGallery.split(a, [DEV, DEV])
    for sh in shards.shards:
        _same_desc(sh)


# ------------------------------------------------------------------------------------------ queries
@pytest.fixture(scope="module")
def mates(sd):
    gal, probes = planted()
    net = _net(sd)
    index = net.enroll(gal, DEV, batch=16, descriptors=True)
    return net, probes, gal, index, net.enroll(probes, DEV, batch=2)


QUERY_KEYS = ("short_idx", "coarse_score", "coarse_all")


def _same_query(got, want, keys=OUT_KEYS + QUERY_KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and tuple(got[k].shape) == tuple(want[k].shape), k
        assert torch.equal(_bits(got[k]) if got[k].dtype == torch.float32 else got[k],
                           _bits(want[k]) if got[k].dtype == torch.float32 else want[k]), k


def test_prescreened_identify_is_selected_identify(mates):
    net, probes, gal, index, pset = mates
    wp = net.packed(DEV)
    dg = index.desc.cpu()
    res = net.identify(probes, index, topk=4, shortlist=4, prescreen=8)
    for p, probe in enumerate(probes):
        r = res[p]
        assert r["pre_idx"].dtype == torch.int32 and tuple(r["pre_idx"].shape) == (8,) and r["pre_idx"].device == DEV
        assert r["pre_score"].dtype == torch.float32 and tuple(r["pre_score"].shape) == (8,)
        assert tuple(r["coarse_all"].shape) == (8,)
        assert bool((r["pre_idx"][1:] > r["pre_idx"][:-1]).all())
        one = net.identify(probe, index, topk=4, shortlist=4, prescreen=8)
        _same_query(one, r, OUT_KEYS + QUERY_KEYS + ("pre_idx", "pre_score"))
        ref = net.identify(probe, index, topk=4, shortlist=4, select=r["pre_idx"])
        assert "pre_idx" not in ref
        _same_query(r, ref)
        # the host ranking: float64 descriptor scores on the device's own descriptors
        yp = net._probe_rows(wp, gallery._ProbeSide(probe, index))
        dq = ops.rows_pool(yp, torch.tensor([0, yp.shape[0]], device=DEV)).cpu()
        s64 = ops.desc_score(dq, dg, dtype=torch.float64)
        err32 = float((ops.desc_score(dq, dg).double() - s64).abs().max())
        top = float(s64.abs().max())
        gate = max(8 * 2.0 ** (np.floor(np.log2(top)) - 23), 8 * err32)
        order = torch.sort(s64[0], descending=True).values
        mate = [e for e, q in MATES.items() if q == p][0]
        print("MEASURE prescreen probe %d: mate %.6f runner-up %.6f gap(8,9) %.3g gate %.3g"
              % (p, float(order[0]), float(order[1]), float(order[7] - order[8]), gate))
        assert float(order[7] - order[8]) > 2 * gate                       # the precondition
        assert torch.equal(r["pre_idx"].cpu(), ops.rank_keep(s64.to(torch.float32), 8)[0])
        assert float((r["pre_score"].cpu().double() - s64[0][r["pre_idx"].cpu().long()]).abs().max()) <= gate
        assert int(s64[0].argmax()) == mate and int(r["short_idx"][0]) == mate
    # K over the selection is clamped; a selection works as it does without a prescreen
    sel = [30, 7, 2, 19, 11]
    few = net.identify(probes[0], index, shortlist=2, prescreen=64, select=sel)
    assert few["pre_idx"].tolist() == [30, 7, 2, 19, 11] and int(few["short_idx"][0]) == 7
    _same_query(few, net.identify(probes[0], index, shortlist=2, select=sel))


def test_prescreened_identify_many(mates):
    net, probes, gal, index, pset = mates
    G = len(gal)
    one = net.identify(probes, index, topk=4, shortlist=4, prescreen=8)
    # group_pairs=4: every probe is a group of its own, as in the per-probe calls below (the same padded boxes)
    for ps in (pset, net.enroll(probes, DEV, batch=2, descriptors=True)):
        res = net.identify_many(ps, index, topk=4, shortlist=4, prescreen=8, group_pairs=4)
        for q, r in enumerate(res):
            assert torch.equal(r["pre_idx"], one[q]["pre_idx"]) and r["pre_idx"].dtype == torch.int32
            assert torch.equal(_bits(r["pre_score"]), _bits(one[q]["pre_score"]))
            assert int(r["short_idx"][0]) == [e for e, p in MATES.items() if p == q][0]
            ref = net.identify_many(ps, index, topk=4, shortlist=4, probe_select=[q], select=r["pre_idx"],
                                    group_pairs=4)[0]
            _same_query(r, ref)
    # de-duplication: no probe keeps itself, K clamps to G - 1
    res = net.identify_many(index, index, topk=2, shortlist=2, prescreen=64, exclude_self=True)
    for q, r in enumerate(res):
        assert r["pre_idx"].tolist() == [e for e in range(G) if e != q]
        assert q not in r["short_idx"].tolist()
    # removed entries are in no list (19 is probe 1's mate: the best descriptor score of that probe)
    holed = net.enroll(gal, DEV, batch=16, descriptors=True)
    holed.remove([3, 19])
    for r in net.identify(probes, holed, shortlist=4, prescreen=8):
        assert not {3, 19} & set(r["pre_idx"].tolist())
    for r in net.identify_many(pset, holed, shortlist=4, prescreen=64):
        assert r["pre_idx"].tolist() == [e for e in range(G) if e not in (3, 19)]


def test_prescreen_refusals(mates, monkeypatch):
    net, probes, gal, index, pset = mates
    plain = net.enroll(gal[:4], DEV, batch=16)
    labelled = net.enroll(gal[:4], DEV, batch=16, subjects=[0, 0, 1, 1], descriptors=True)
    shards = ShardedGallery.split(index, [DEV, DEV])

    def boom(*a, **k):
        raise AssertionError("a launch before the refusal")

    monkeypatch.setattr(_lib, "call", boom)
    for call in (lambda **kw: net.identify(probes[0], kw.pop("index", index), **kw),
                 lambda **kw: net.identify_many(pset, kw.pop("index", index), **kw)):
        with pytest.raises(_lib.FpmError, match="prescreen needs a shortlist"):
            call(prescreen=8)
        for k in (3, 8.0, "8", True):
            with pytest.raises(_lib.FpmError, match="integer >= shortlist"):
                call(shortlist=4, prescreen=k)
        with pytest.raises(_lib.FpmError, match="add_descriptors.*descriptors=True"):
            call(index=plain, shortlist=2, prescreen=4)
        with pytest.raises(_lib.FpmError, match="by='subject'"):
            call(index=labelled, shortlist=2, prescreen=4, by="subject")
        with pytest.raises(_lib.FpmError, match="ShardedGallery"):
            call(index=shards, shortlist=2, prescreen=4)


# -------------------------------------------------------------------------------------------- C-ABI
def test_c_abi_entry_points():
    lib = _lib.load()
    P = ctypes.c_void_p
    st = P(torch.cuda.current_stream(DEV).cuda_stream)
    y, off = pool_case()
    y_d, off_d = y.to(DEV), off.to(DEV)
    E = len(POOL_NS)
    d = torch.zeros(E, 768, dtype=torch.bfloat16, device=DEV)
    assert lib.fpm_rows_pool(P(y_d.data_ptr()), y.shape[0], P(off_d.data_ptr()), 0, E, P(d.data_ptr()), st) == 0
    assert torch.equal(_bits(d.cpu()), _bits(ops.rows_pool(y, off)))
    assert lib.fpm_rows_pool(P(y_d.data_ptr()), y.shape[0], P(off_d.data_ptr()), 3, 2, P(d.data_ptr()), st) != 0
    assert b"rows_pool: bad sizes" in lib.fpm_last_error()
    assert lib.fpm_rows_pool(P(y_d.data_ptr() + 4), y.shape[0] - 1, P(off_d.data_ptr()), 0, 1, P(d.data_ptr()), st) != 0
    assert b"aligned" in lib.fpm_last_error()

    sc = torch.full((E, E), float("nan"), device=DEV)
    assert lib.fpm_desc_score(P(d.data_ptr()), E, P(d.data_ptr()), E, P(0), E, P(sc.data_ptr()), st) == 0
    assert torch.equal(_bits(sc), _bits(ops.desc_score(d, d)))
    assert lib.fpm_desc_score(P(d.data_ptr()), E, P(d.data_ptr()), E, P(0), E - 1, P(sc.data_ptr()), st) != 0
    assert b"desc_score: without idx" in lib.fpm_last_error()
    assert lib.fpm_desc_score(P(d.data_ptr()), -1, P(d.data_ptr()), E, P(0), E, P(sc.data_ptr()), st) != 0
    assert b"desc_score: bad sizes" in lib.fpm_last_error()

    s = keep_scores(2, 4000, 9)
    s_d = s.to(DEV)
    k = 1300
    keep = torch.empty(2, k, dtype=torch.int32, device=DEV)
    wsb = int(lib.fpm_rank_keep_ws_bytes(2, 4000))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    args = lambda k_, wsb_: (P(s_d.data_ptr()), 4000, 2, 4000, k_, P(keep.data_ptr()), P(ws.data_ptr()), wsb_, st)
    assert lib.fpm_rank_keep(*args(k, wsb)) == 0
    assert torch.equal(keep.cpu(), ops.rank_keep(s, k))
    for bad in (0, 4001):
        assert lib.fpm_rank_keep(*args(bad, wsb)) != 0 and b"rank_keep: k" in lib.fpm_last_error()
    assert lib.fpm_rank_keep(*args(k, wsb - 8)) != 0 and b"workspace" in lib.fpm_last_error()
    assert lib.fpm_rank_keep(P(s_d.data_ptr()), 3999, 2, 4000, k, P(keep.data_ptr()), P(ws.data_ptr()), wsb, st) != 0
    assert b"rank_keep: bad sizes" in lib.fpm_last_error()

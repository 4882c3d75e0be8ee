"""The streamed coarse score on the GPU (boxes of up to 600 keypoints): ``fpm_coarse_score_stream``
against float64 over the shape set of ``test_coarse_stream_cpu.py``, its composition independence
(alone and routed per pair under ``coarse="any"``, where all three coarse kernels run in one call),
``Net.identify(shortlist=M, coarse="stream")`` against the selected identify (bit for bit), planted
mates over 256 keypoints, the refusals and the C-ABI.

Gate of the kernel test (that of ``test_shortlist_gpu.py``): ``ref`` is the host statement of the score
in float64 on bit-identical operands, ``ref32`` the same in float32, ``err32 = max |ref32 - ref|``
over a case's whole shape set.  The device must stay within ``max(8 ulp32(max |ref|), 8 err32)``; the
runs at 1, 2 and 3 Sinkhorn steps are held to the same figure.

MEASURED (the table below): the largest device error, err32 and their ratio per case, on an MI355X.
"""
import ctypes

import numpy as np
import pytest
import torch

from fpm import _lib, gallery, ops, synth
from test_coarse_stream_cpu import STREAM_SHAPES, stream_case
from test_coarse_wide_cpu import SCALES
from test_shortlist_cpu import coefficients, state_dicts
from test_shortlist_gpu import OUT_KEYS, _bits, _net, noisy_copy

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

MEASURED = {
    # case: (device_err, err32, device_err / err32, gate); scores 0.193-0.194 (flat), 0.817-2.04 (spread)
    "flat": (3.68e-08, 4.22e-08, 0.87, 3.38e-07),
    "spread": (1.55e-06, 9.51e-07, 1.63, 7.61e-06),
    # spread, (300, 600) / (600, 300) at iters = 1, 2, 3: device error 6.7e-7 / 5.2e-8, 6.3e-7 / 8.1e-7,
    # 1.2e-7 / 1.2e-7 under the same 7.61e-06
}


@pytest.fixture(scope="module")
def sds():
    return state_dicts()


def _gate(name):
    """(ref, ref32, err32, gate) of a case's whole shape set at the default 10 steps."""
    _, _, probes = stream_case(name)
    ref = torch.cat([p[4] for p in probes])
    ref32 = torch.cat([p[5].double() for p in probes])
    err32 = float((ref32 - ref).abs().max())
    ulp = 2.0 ** (np.floor(np.log2(float(ref.abs().max()))) - 23)
    return ref, ref32, err32, max(8 * ulp, 8 * err32)


# ------------------------------------------------------------------------------ kernel vs float64
@pytest.mark.parametrize("name", sorted(SCALES))
def test_stream_kernel_vs_float64(name):
    y, row_off, probes = stream_case(name)
    y_d, off_d = y.to(DEV), row_off.to(DEV)
    devs, seen = [], set()
    for n0, yp, idx, coef, _, _ in probes:
        out = torch.full((idx.numel(),), float("nan"), device=DEV)
        ops.coarse_score_stream(y_d, off_d, idx.to(DEV), yp.to(DEV), coef.to(DEV), out=out)
        devs.append(out.cpu().double())
        assert float(out[0]) == float(out[-1])                                    # the entry listed twice
        seen |= {(n0, int(row_off[e + 1] - row_off[e])) for e in idx.tolist()}
    assert set(STREAM_SHAPES) <= seen
    dev = torch.cat(devs)
    ref, _, err32, gate = _gate(name)
    assert bool(torch.isfinite(dev).all())
    err = float((dev - ref).abs().max())
    print("MEASURE coarse_stream %s err=%.3g err32=%.3g ratio=%.3g gate=%.3g scores=[%.3g, %.3g]"
          % (name, err, err32, err / err32, gate, float(ref.min()), float(ref.max())))
    assert err <= gate, "coarse_stream %s: device error %.3g over the gate %.3g (err32 %.3g)" % (name, err, gate, err32)


@pytest.mark.parametrize("iters", [1, 2, 3])
def test_stream_kernel_few_steps(iters):
    """The re-base step alone, one potential step and an odd count, on the pairs with 300 dummy rows."""
    y, row_off, probes = stream_case("spread")
    _, _, err32, gate = _gate("spread")
    ns = (row_off[1:] - row_off[:-1]).tolist()
    for n0, ng in ((300, 600), (600, 300)):
        _, yp, _, coef, _, _ = [p for p in probes if p[0] == n0][0]
        idx = torch.tensor([ns.index(ng)], dtype=torch.int32)
        ref = ops.coarse_score_stream(y, row_off, idx, yp, coef[:1], iters=iters, dtype=torch.float64)
        out = ops.coarse_score_stream(y.to(DEV), row_off.to(DEV), idx.to(DEV), yp.to(DEV), coef[:1].to(DEV), iters=iters)
        err = float((out.cpu().double() - ref).abs().max())
        print("MEASURE coarse_stream spread (%d, %d) iters=%d err=%.3g gate=%.3g score=%.6g"
              % (n0, ng, iters, err, gate, float(ref[0])))
        assert err <= gate, (n0, ng, iters, err, gate)


# ---------------------------------------------------------- planted-mate gallery over 256 keypoints
MATES = {4: 0, 8: 1, 10: 2}            # gallery entry -> probe
PROBE_N = (300, 600, 259)              # the mates have 297, 597 and 256 keypoints
GALLERY_N = (100, 600, 280, 128, 513, 257, 350, 200, 450, 300, 160, 590)


def planted():
    gal = [synth.make_graph(45, p, 1, n) for p, n in enumerate(GALLERY_N)]
    probes = [synth.make_graph(45, p, 0, n) for p, n in enumerate(PROBE_N)]
    for e, p in MATES.items():
        gal[e] = noisy_copy(probes[p], 3000 + e)
    return gal, probes


@pytest.fixture(scope="module")
def mates(sds):
    gal, probes = planted()
    net = _net(sds["spread"])
    index = net.enroll(gal, DEV, batch=4)
    return net, probes, gal, index


def _independent(net, probe, other, index, G, coarse):
    """An entry's score is the same bits alone, in the full launch, in a permuted selection walked in
    other chunks and beside another probe.  -> the full launch's scores."""
    full = net.coarse_scores(probe, index, coarse=coarse)
    assert tuple(full.shape) == (1, G) and full.dtype == torch.float32 and full.device == index.device
    assert bool(torch.isfinite(full).all())
    perm = torch.randperm(G, generator=torch.Generator().manual_seed(3))
    mixed = gallery.coarse_scores(net, probe, index, select=perm, chunk=5, coarse=coarse)
    assert torch.equal(_bits(mixed[0]), _bits(full[0][perm.to(DEV)]))
    for e in (0, 1, 5, G - 1):
        alone = net.coarse_scores(probe, index, select=[e], coarse=coarse)
        assert torch.equal(_bits(alone[0]), _bits(full[0, e:e + 1])), e
    both = net.coarse_scores([other, probe], index, coarse=coarse)
    assert torch.equal(_bits(both[1]), _bits(full[0]))
    return full[0]


def test_stream_composition_independence(mates):
    net, probes, gal, index = mates
    ns = [g["n"] for g in gal]
    assert len(gal) == 12 and min(ns) <= 128 and max(ns) == 600 and any(256 < n <= 300 for n in ns)
    assert probes[0]["n"] == 300
    full = _independent(net, probes[0], probes[2], index, len(gal), "stream")
    # a probe over 256 keypoints under "any": every pair through the stream kernel
    assert torch.equal(_bits(net.coarse_scores(probes[0], index, coarse="any")[0]), _bits(full))


def test_any_routes_per_pair(mates):
    net, probes, gal, index = mates
    small = synth.make_graph(45, 7, 0, 120)
    rt = gallery.coarse_routes(120, index.n, "any")
    assert sorted(set(rt.tolist())) == [0, 1, 2]               # all three kernels run in one call
    anyr = _independent(net, small, probes[2], index, len(gal), "any")
    fits = [torch.nonzero(rt <= k).view(-1) for k in (0, 1)]
    stream = net.coarse_scores(small, index, coarse="stream")[0]
    wide = net.coarse_scores(small, index, select=fits[1], coarse="wide")[0]
    fused = net.coarse_scores(small, index, select=fits[0])[0]
    want = stream.clone()
    want[fits[1].to(DEV)] = wide
    want[fits[0].to(DEV)] = fused
    assert torch.equal(_bits(anyr), _bits(want))
    # the kernels agree to rounding on the boxes they share
    # (each is held within 1e-5 of the float64 scores of such a gallery by its planted-mate test)
    assert float((stream[fits[1].to(DEV)] - wide).abs().max()) < 2e-5
    assert float((stream[fits[0].to(DEV)] - fused).abs().max()) < 2e-5
    pos = torch.tensor([fits[1].tolist().index(e) for e in fits[0].tolist()], device=DEV)
    assert float((wide[pos] - fused).abs().max()) < 2e-5


# -------------------------------------------------------------- shortlisted identify = selected identify
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stream_shortlisted_identify_is_selected_identify(dtype, sds):
    ns = np.random.default_rng(5).integers(260, 401, 8)
    probe = synth.make_graph(46, 0, 0, 300)
    gal = [synth.make_graph(46, p, 1, int(n)) for p, n in enumerate(ns)]
    net = _net(sds["flat"], dtype)
    index = net.enroll(gal, DEV, batch=4)
    res = net.identify(probe, index, topk=3, shortlist=3, chunks=2, coarse="stream")
    assert res["short_idx"].dtype == torch.int32 and tuple(res["short_idx"].shape) == (3,)
    assert tuple(res["coarse_all"].shape) == (len(gal),)
    ref = net.identify(probe, index, topk=3, select=res["short_idx"], chunks=2)
    for k in OUT_KEYS:
        assert torch.equal(res[k], ref[k]), k
    hi, hs = ops.rank_select(res["coarse_all"].cpu().view(1, -1), 3)
    assert torch.equal(res["short_idx"].cpu(), hi[0])
    assert torch.equal(_bits(res["coarse_score"].cpu()), _bits(hs[0]))
    assert torch.equal(_bits(res["coarse_all"]), _bits(net.coarse_scores(probe, index, coarse="stream")[0]))


# ------------------------------------------------------------------------------------ planted mate
def test_planted_mate_over_256_is_shortlisted(mates, sds):
    net, probes, gal, index = mates
    wp = net.packed(DEV)
    y, off = index.y.cpu(), index.row_off_host
    idx = torch.arange(len(gal), dtype=torch.int32)
    assert [gal[e]["n"] for e in MATES] == [297, 597, 256]
    res = net.identify(probes, index, topk=4, shortlist=4, coarse="stream")
    for p, probe in enumerate(probes):
        # the CPU ranking, float64, on the device's own operands
        yp = net._probe_rows(wp, gallery._ProbeSide(probe, index)).cpu()
        coef = coefficients(probe["w"], [g["w"] for g in gal], sds["spread"])
        coef_d = torch.empty(len(gal), 768, device=DEV)
        w0 = torch.from_numpy(probe["w"]).to(DEV).view(1, -1).expand(len(gal), -1).contiguous()
        ops.coef_tanh(ops.global_weights(w0, index.w), wp["aff_wT"], wp["aff_b"], coef_d)
        assert float((coef_d.cpu() - coef).abs().max()) < 1e-5
        sc = ops.coarse_score_stream(y, off, idx, yp, coef_d.cpu(), dtype=torch.float64)
        order = torch.argsort(sc, descending=True, stable=True)
        mate = [e for e, q in MATES.items() if q == p][0]
        top = sc[order]
        print("MEASURE stream mate probe %d: top5 %s at %s"
              % (p, [round(float(v), 6) for v in top[:5]], order[:5].tolist()))
        # the precondition, on the CPU ranking: the mate first, the top five pairwise more than 1e-5 apart
        assert int(order[0]) == mate
        assert float((top[:4] - top[1:5]).min()) > 1e-5
        assert res[p]["short_idx"].tolist() == order[:4].tolist()
        assert int(res[p]["short_idx"][0]) == mate
        assert float((res[p]["coarse_all"].cpu().double() - sc).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------- refusals
def test_stream_refusals(mates):
    net, probes, gal, index = mates
    probe = probes[0]
    big = synth.make_graph(45, 0, 0, 601)
    index_big = net.enroll([gal[0], synth.make_graph(45, 1, 1, 601)], DEV)
    for coarse in ("stream", "any"):
        with pytest.raises(_lib.FpmError, match="COARSE_STREAM_NMAX"):
            net.identify(big, index, shortlist=2, coarse=coarse)
        with pytest.raises(_lib.FpmError, match=r"COARSE_STREAM_NMAX = 600 \(identify without a shortlist has no such "
                                                r"bound\)$"):
            net.coarse_scores(big, index, coarse=coarse)
        with pytest.raises(_lib.FpmError, match="COARSE_STREAM_NMAX"):
            net.identify(probe, index_big, shortlist=1, coarse=coarse)
        assert net.identify(probe, index_big, shortlist=1, select=[0], coarse=coarse)["short_idx"].tolist() == [0]
    for call in (lambda: net.coarse_scores(probe, index, coarse="narrow"),
                 lambda: net.identify(probe, index, shortlist=2, coarse="narrow"),
                 lambda: net.identify(probe, index, coarse=None)):
        with pytest.raises(_lib.FpmError, match=r"coarse must be one of \('fused', 'wide', 'auto', 'stream', 'any'\)"):
            call()
    # the earlier routes keep their bounds and their messages
    with pytest.raises(_lib.FpmError, match="COARSE_NMAX = 128"):
        net.coarse_scores(probe, index)
    index257 = net.enroll([gal[0], gal[5]], DEV)
    assert gal[5]["n"] == 257
    with pytest.raises(_lib.FpmError, match="COARSE_WIDE_NMAX = 256.*without a shortlist"):
        net.coarse_scores(synth.make_graph(45, 7, 0, 120), index257, coarse="auto")
    # the low-level op: nothing is launched, the output stays as it was
    yp = torch.zeros(4, 768, device=DEV)
    coef = torch.zeros(2, 768, device=DEV)
    idx = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    out = torch.full((2,), float("nan"), device=DEV)
    yb, ob = index_big.y, index_big.row_off
    bad = [
        (dict(idx=idx.long()), "int32"),
        (dict(idx=torch.stack([idx, idx], 1)[:, 0]), "contiguous"),
        (dict(idx=torch.tensor([0, 2], dtype=torch.int32, device=DEV)), "outside"),
        (dict(), "COARSE_STREAM_NMAX"),                            # entry 1 has 601 keypoints
        (dict(idx=idx[:1].repeat(2), yp=torch.zeros(601, 768, device=DEV)), "COARSE_STREAM_NMAX"),
        (dict(idx=idx.cpu()), "is on"),
    ]
    for kw, msg in bad:
        a = dict(idx=idx, yp=yp)
        a.update(kw)
        with pytest.raises(_lib.FpmError, match=msg):
            ops.coarse_score_stream(yb, ob, a["idx"], a["yp"], coef, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------- C-ABI
def test_stream_c_abi_entry_point(mates):
    net, probes, gal, index = mates
    lib = _lib.load()
    P = ctypes.c_void_p
    st = P(torch.cuda.current_stream(DEV).cuda_stream)
    wp = net.packed(DEV)
    probe = probes[0]
    yp = net._probe_rows(wp, gallery._ProbeSide(probe, index))
    n0 = int(yp.shape[0])
    B = 5
    idx = torch.tensor([4, 1, 0, 1, 11], dtype=torch.int32, device=DEV)
    ngmax = max(gal[e]["n"] for e in idx.tolist())
    coef = torch.empty(B, 768, device=DEV)
    w0 = torch.from_numpy(probe["w"]).to(DEV).view(1, -1).expand(B, -1).contiguous()
    ops.coef_tanh(ops.global_weights(w0, index.w[idx.long()]), wp["aff_wT"], wp["aff_b"], coef)
    out = torch.full((B,), float("nan"), device=DEV)
    wsb_of = lambda b, a, g: int(lib.fpm_coarse_score_stream_ws_bytes(b, a, g))
    wsb = wsb_of(B, n0, ngmax)
    assert n0 == 300 and ngmax == 600 and wsb == B * 300 * 600 * 4
    # monotone in every argument, constant from 256 pairs on, at most 800 MiB
    assert wsb_of(100000, 600, 600) == wsb_of(256, 600, 600) == 256 * 600 * 600 * 4 <= 800 << 20
    for b, a, g in ((1, 1, 1), (5, 300, 400), (255, 599, 600), (256, 600, 599), (7, 130, 131)):
        here = wsb_of(b, a, g)
        assert 0 < here <= min(wsb_of(b + 1, a, g), wsb_of(b, a + 1, g), wsb_of(b, a, g + 1)) <= 800 << 20, (b, a, g)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)

    def call(n0_, wsb_):
        out.fill_(float("nan"))
        return lib.fpm_coarse_score_stream(P(index.y.data_ptr()), P(index.row_off.data_ptr()), P(idx.data_ptr()),
                                           index.G, B, P(yp.data_ptr()), n0_, P(coef.data_ptr()), 10, 0.01,
                                           P(out.data_ptr()), P(ws.data_ptr()), wsb_, st)

    assert call(n0, wsb) == 0
    ref = net.coarse_scores(probe, index, select=idx.cpu(), coarse="stream")
    assert torch.equal(_bits(out), _bits(ref[0]))
    assert call(601, wsb) != 0 and b"COARSE_STREAM_NMAX" in lib.fpm_last_error()
    # a workspace under the call's own minimum (no entry at all would fit) is refused on the host ...
    assert call(n0, wsb_of(B, n0, 1) - 16) != 0 and b"workspace" in lib.fpm_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # ... and one 16 bytes short of what these entries need serves the entries that still fit its
    # slots, the same bits, and gives NaN to the 600-keypoint ones (their rows are not read)
    assert call(n0, wsb - 16) == 0
    big = torch.tensor([gal[e]["n"] == 600 for e in idx.tolist()], device=DEV)
    assert bool(torch.isnan(out[big]).all()) and int(big.sum()) == 2
    assert torch.equal(_bits(out[~big]), _bits(ref[0][~big]))

"""The wide coarse score on the GPU (boxes of up to 256 keypoints): ``fpm_coarse_score_wide`` against
float64 over the shape set of ``test_coarse_wide_cpu.py``, its composition independence (alone and
routed per pair under ``coarse="auto"``), ``Net.identify(shortlist=M, coarse="wide")`` against the
selected identify (bit for bit), a planted mate over 128 keypoints, the refusals and the C-ABI.

Gate of the kernel test (that of ``test_shortlist_gpu.py``): ``ref`` is the host statement of the score
in float64 on bit-identical operands, ``ref32`` the same in float32, ``err32 = max |ref32 - ref|``
over a case's whole shape set.  The device must stay within ``max(8 ulp32(max |ref|), 8 err32)``.

MEASURED (the table below): the largest device error, err32 and their ratio per case, on an MI355X.
"""
import ctypes

import numpy as np
import pytest
import torch

from fpm import _lib, gallery, ops, synth
from test_coarse_wide_cpu import SCALES, WIDE_SHAPES, synthetic_case
from test_shortlist_cpu import coefficients, state_dicts
from test_shortlist_gpu import OUT_KEYS, _bits, _net, noisy_copy

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

MEASURED = {
    # case: (device_err, err32, device_err / err32, gate); scores 0.193-0.195 (flat), 0.182-1.78 (spread)
    "flat": (5.57e-08, 3.57e-08, 1.56, 2.85e-07),
    "spread": (2.71e-06, 1.96e-06, 1.39, 1.56e-05),
}


@pytest.fixture(scope="module")
def sds():
    return state_dicts()


# ------------------------------------------------------------------------------ kernel vs float64
@pytest.mark.parametrize("name", sorted(SCALES))
def test_wide_kernel_vs_float64(name):
    y, row_off, probes = synthetic_case(name)
    y_d, off_d = y.to(DEV), row_off.to(DEV)
    devs, refs, refs32, seen = [], [], [], set()
    for n0, yp, idx, coef in probes:
        out = torch.full((idx.numel(),), float("nan"), device=DEV)
        ops.coarse_score_wide(y_d, off_d, idx.to(DEV), yp.to(DEV), coef.to(DEV), out=out)
        devs.append(out.cpu().double())
        refs.append(ops.coarse_score_wide(y, row_off, idx, yp, coef, dtype=torch.float64))
        refs32.append(ops.coarse_score_wide(y, row_off, idx, yp, coef).double())
        assert float(out[0]) == float(out[-1])                                    # the entry listed twice
        seen |= {(n0, int(row_off[e + 1] - row_off[e])) for e in idx.tolist()}
    assert set(WIDE_SHAPES) <= seen
    dev, ref, ref32 = torch.cat(devs), torch.cat(refs), torch.cat(refs32)
    assert bool(torch.isfinite(dev).all())
    err32 = float((ref32 - ref).abs().max())
    top = float(ref.abs().max())
    ulp = 2.0 ** (np.floor(np.log2(top)) - 23)
    gate = max(8 * ulp, 8 * err32)
    err = float((dev - ref).abs().max())
    print("MEASURE coarse_wide %s err=%.3g err32=%.3g ratio=%.3g gate=%.3g scores=[%.3g, %.3g]"
          % (name, err, err32, err / err32, gate, float(ref.min()), float(ref.max())))
    assert err <= gate, "coarse_wide %s: device error %.3g over the gate %.3g (err32 %.3g)" % (name, err, gate, err32)


# ---------------------------------------------------------- planted-mate gallery over 128 keypoints
MATES = {5: 0, 11: 1, 14: 2}           # gallery entry -> probe
PROBE_N = (160, 256, 131)              # the last mate has 128 keypoints under a 131-keypoint probe


def planted():
    ns = np.random.default_rng(1).integers(100, 257, 16)
    ns[3] = 256
    gal = [synth.make_graph(43, p, 1, int(n)) for p, n in enumerate(ns)]
    probes = [synth.make_graph(43, p, 0, n) for p, n in enumerate(PROBE_N)]
    for e, p in MATES.items():
        gal[e] = noisy_copy(probes[p], 2000 + e)
    return gal, probes


@pytest.fixture(scope="module")
def mates(sds):
    gal, probes = planted()
    net = _net(sds["spread"])
    index = net.enroll(gal, DEV, batch=8)
    return net, probes, gal, index


def _independent(net, probe, other, index, G, coarse):
    """An entry's score is the same bits alone, in the full launch, in a permuted selection walked in
    other chunks and beside another probe.  -> the full launch's scores."""
    full = net.coarse_scores(probe, index, coarse=coarse)
    assert tuple(full.shape) == (1, G) and full.dtype == torch.float32 and full.device == index.device
    assert bool(torch.isfinite(full).all())
    perm = torch.randperm(G, generator=torch.Generator().manual_seed(3))
    mixed = gallery.coarse_scores(net, probe, index, select=perm, chunk=7, coarse=coarse)
    assert torch.equal(_bits(mixed[0]), _bits(full[0][perm.to(DEV)]))
    for e in (0, 3, 14, G - 1):
        alone = net.coarse_scores(probe, index, select=[e], coarse=coarse)
        assert torch.equal(_bits(alone[0]), _bits(full[0, e:e + 1])), e
    both = net.coarse_scores([other, probe], index, coarse=coarse)
    assert torch.equal(_bits(both[1]), _bits(full[0]))
    return full[0]


def test_wide_composition_independence(mates):
    net, probes, gal, index = mates
    ns = [g["n"] for g in gal]
    assert min(ns) <= 128 and max(ns) == 256 and probes[0]["n"] == 160
    _independent(net, probes[0], probes[2], index, len(gal), "wide")
    # a probe over 128 keypoints under "auto": every pair through the wide kernel
    assert torch.equal(_bits(net.coarse_scores(probes[0], index, coarse="auto")),
                       _bits(net.coarse_scores(probes[0], index, coarse="wide")))


def test_auto_routes_per_pair(mates):
    net, probes, gal, index = mates
    small = synth.make_graph(43, 7, 0, 120)
    fits = [e for e, g in enumerate(gal) if g["n"] <= ops.COARSE_NMAX]
    assert 0 < len(fits) < len(gal)                            # both kernels run in one call
    auto = _independent(net, small, probes[2], index, len(gal), "auto")
    wide = net.coarse_scores(small, index, coarse="wide")[0]
    fused = net.coarse_scores(small, index, select=fits)[0]
    want = wide.clone()
    want[torch.tensor(fits, device=DEV)] = fused
    assert torch.equal(_bits(auto), _bits(want))
    # the two kernels agree to rounding on the boxes both take
    # (each is held within 1e-5 of the float64 scores of such a gallery by its planted-mate test)
    assert float((wide[torch.tensor(fits, device=DEV)] - fused).abs().max()) < 2e-5


# -------------------------------------------------------------- shortlisted identify = selected identify
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_wide_shortlisted_identify_is_selected_identify(dtype, sds):
    ns = np.random.default_rng(5).integers(100, 201, 8)
    probe = synth.make_graph(44, 0, 0, 140)
    gal = [synth.make_graph(44, p, 1, int(n)) for p, n in enumerate(ns)]
    net = _net(sds["flat"], dtype)
    index = net.enroll(gal, DEV, batch=4)
    res = net.identify(probe, index, topk=3, shortlist=3, chunks=2, coarse="wide")
    assert res["short_idx"].dtype == torch.int32 and tuple(res["short_idx"].shape) == (3,)
    assert tuple(res["coarse_all"].shape) == (len(gal),)
    ref = net.identify(probe, index, topk=3, select=res["short_idx"], chunks=2)
    for k in OUT_KEYS:
        assert torch.equal(res[k], ref[k]), k
    hi, hs = ops.rank_select(res["coarse_all"].cpu().view(1, -1), 3)
    assert torch.equal(res["short_idx"].cpu(), hi[0])
    assert torch.equal(_bits(res["coarse_score"].cpu()), _bits(hs[0]))
    assert torch.equal(_bits(res["coarse_all"]), _bits(net.coarse_scores(probe, index, coarse="wide")[0]))


# ------------------------------------------------------------------------------------ planted mate
def test_planted_mate_over_128_is_shortlisted(mates, sds):
    net, probes, gal, index = mates
    wp = net.packed(DEV)
    y, off = index.y.cpu(), index.row_off_host
    idx = torch.arange(len(gal), dtype=torch.int32)
    assert gal[14]["n"] == 128 and probes[2]["n"] == 131
    res = net.identify(probes, index, topk=4, shortlist=4, coarse="wide")
    for p, probe in enumerate(probes):
        # the CPU ranking, float64, on the device's own operands
        yp = net._probe_rows(wp, gallery._ProbeSide(probe, index)).cpu()
        coef = coefficients(probe["w"], [g["w"] for g in gal], sds["spread"])
        coef_d = torch.empty(len(gal), 768, device=DEV)
        w0 = torch.from_numpy(probe["w"]).to(DEV).view(1, -1).expand(len(gal), -1).contiguous()
        ops.coef_tanh(ops.global_weights(w0, index.w), wp["aff_wT"], wp["aff_b"], coef_d)
        assert float((coef_d.cpu() - coef).abs().max()) < 1e-5
        sc = ops.coarse_score_wide(y, off, idx, yp, coef_d.cpu(), dtype=torch.float64)
        order = torch.argsort(sc, descending=True, stable=True)
        mate = [e for e, q in MATES.items() if q == p][0]
        top = sc[order]
        print("MEASURE wide mate probe %d: top5 %s at %s"
              % (p, [round(float(v), 6) for v in top[:5]], order[:5].tolist()))
        # the precondition, on the CPU ranking: mate first by more than 1.0, ranks 1..5 well apart
        assert int(order[0]) == mate and float(top[0] - top[1]) > 1.0
        assert float((top[:4] - top[1:5]).min()) > 1e-5
        assert res[p]["short_idx"].tolist() == order[:4].tolist()
        assert int(res[p]["short_idx"][0]) == mate
        assert float((res[p]["coarse_all"].cpu().double() - sc).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------- refusals
def test_wide_refusals(mates):
    net, probes, gal, index = mates
    probe = probes[0]
    big = synth.make_graph(43, 0, 0, 257)
    index_big = net.enroll([gal[0], synth.make_graph(43, 1, 1, 257)], DEV)
    for coarse in ("wide", "auto"):
        with pytest.raises(_lib.FpmError, match="COARSE_WIDE_NMAX"):
            net.identify(big, index, shortlist=2, coarse=coarse)
        with pytest.raises(_lib.FpmError, match="COARSE_WIDE_NMAX.*without a shortlist"):
            net.coarse_scores(big, index, coarse=coarse)
        with pytest.raises(_lib.FpmError, match="COARSE_WIDE_NMAX"):
            net.identify(probe, index_big, shortlist=1, coarse=coarse)
        assert net.identify(probe, index_big, shortlist=1, select=[0], coarse=coarse)["short_idx"].tolist() == [0]
    for call in (lambda: net.coarse_scores(probe, index, coarse="narrow"),
                 lambda: net.identify(probe, index, shortlist=2, coarse="narrow"),
                 lambda: net.identify(probe, index, coarse=None)):
        with pytest.raises(_lib.FpmError, match="coarse must be one of"):
            call()
    # the default route keeps its bound and its message
    with pytest.raises(_lib.FpmError, match="COARSE_NMAX = 128"):
        net.coarse_scores(probe, index)
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
        (dict(), "COARSE_WIDE_NMAX"),                              # entry 1 has 257 keypoints
        (dict(idx=idx[:1].repeat(2), yp=torch.zeros(257, 768, device=DEV)), "COARSE_WIDE_NMAX"),
        (dict(idx=idx.cpu()), "is on"),
    ]
    for kw, msg in bad:
        a = dict(idx=idx, yp=yp)
        a.update(kw)
        with pytest.raises(_lib.FpmError, match=msg):
            ops.coarse_score_wide(yb, ob, a["idx"], a["yp"], coef, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------- C-ABI
def test_wide_c_abi_entry_point(mates):
    net, probes, gal, index = mates
    lib = _lib.load()
    P = ctypes.c_void_p
    st = P(torch.cuda.current_stream(DEV).cuda_stream)
    wp = net.packed(DEV)
    probe = probes[0]
    yp = net._probe_rows(wp, gallery._ProbeSide(probe, index))
    B = 5
    idx = torch.tensor([4, 3, 0, 3, 14], dtype=torch.int32, device=DEV)
    coef = torch.empty(B, 768, device=DEV)
    w0 = torch.from_numpy(probe["w"]).to(DEV).view(1, -1).expand(B, -1).contiguous()
    ops.coef_tanh(ops.global_weights(w0, index.w[idx.long()]), wp["aff_wT"], wp["aff_b"], coef)
    out = torch.full((B,), float("nan"), device=DEV)
    wsb = int(lib.fpm_coarse_score_wide_ws_bytes(B))
    assert wsb == B * 256 * 256 * 4 and int(lib.fpm_coarse_score_wide_ws_bytes(100000)) == 256 * 256 * 256 * 4
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)

    def call(n0, wsb_):
        return lib.fpm_coarse_score_wide(P(index.y.data_ptr()), P(index.row_off.data_ptr()), P(idx.data_ptr()),
                                         index.G, B, P(yp.data_ptr()), n0, P(coef.data_ptr()), 10, 0.01,
                                         P(out.data_ptr()), P(ws.data_ptr()), wsb_, st)

    assert call(int(yp.shape[0]), wsb) == 0
    ref = net.coarse_scores(probe, index, select=idx.cpu(), coarse="wide")
    assert torch.equal(_bits(out), _bits(ref[0]))
    assert call(257, wsb) != 0 and b"COARSE_WIDE_NMAX" in lib.fpm_last_error()
    assert call(int(yp.shape[0]), wsb - 16) != 0 and b"workspace" in lib.fpm_last_error()

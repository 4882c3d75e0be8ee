"""Shortlisted 1:N identification on the GPU: the fused coarse-score kernel against float64 and its
composition independence, ``ops.rank_select`` against its host path, ``Net.identify(shortlist=M)``
against the selected identify (bit for bit), a planted mate, the refusals and the C-ABI.

Gate of the kernel test (the convention of ``test_afau_stages.py``): ``ref`` is the host statement of
the score (``ops.coarse_score`` on CPU tensors) in float64 on bit-identical operands, ``ref32`` the
same in float32, ``err32 = max |ref32 - ref|`` over a case (one state dict's whole shape set: a
single pair's err32 can be 1e-10 by luck).  The device must stay within
``max(8 ulp32(max |ref|), 8 err32)``.

MEASURED (the table below): the largest device error, err32 and their ratio per case, on an MI355X.
"""
import ctypes

import numpy as np
import pytest
import torch

import fpm
from fpm import _lib, gallery, ops, params, synth
from test_gallery_gpu import CASES
from test_shortlist_cpu import (ENTRY_NS, PROBE_NS, SHAPES, coefficients, ragged_case, rank_scores, state_dicts)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
OUT_KEYS = ("s", "ss", "ds_mat", "perm_mat", "k_prob", "cls_prob", "top_idx", "top_score")

# The keys of one probe's result dict for each query form, as recorded from a run of the commit before the query
# stages were shared (the planted gallery of 40 entries, three probes, fp32 and bf16 nets: the same sets).
# FORWARD_KEYS are the forward's own in every run.  FORWARD_RUN_KEYS it adds by how it runs, not by the query form:
# "ss64" (the fp64 k chain) on boxes within ``Net.k_f64_nmax``, "Kp" and "coef" when it runs in one piece (not with
# ``chunks``).  On the planted gallery every form carried all three; a call site whose forward runs otherwise says
# which it expects (``run_keys``).  QUERY_KEYS: what the query layer adds, by (call, by, shortlisted).  One
# asymmetry is on purpose: identify_many(by="subject") without a shortlist carries short_idx / short_off (its ragged
# pair lists), identify(by="subject") without one does not.
FORWARD_KEYS = {"cls_logits", "cls_loss", "cls_prob", "ds_mat", "k_prob", "ks_error", "ks_loss", "lsa", "perm_mat", "s",
                "sk_steps", "ss"}
FORWARD_RUN_KEYS = {"Kp", "coef", "ss64"}
QUERY_KEYS = {
    ("identify", None, False): {"top_idx", "top_score"},
    ("identify", None, True): {"top_idx", "top_score", "short_idx", "coarse_score", "coarse_all"},
    ("identify", "subject", False): {"top_idx", "top_score", "subjects", "subject_score", "top_subject"},
    ("identify", "subject", True): {"top_idx", "top_score", "subjects", "subject_score", "top_subject", "short_subject",
                                    "coarse_subject_score", "coarse_all", "short_idx", "short_off"},
    ("identify_many", None, False): {"group", "top_idx", "top_score"},
    ("identify_many", None, True): {"group", "top_idx", "top_score", "short_idx", "coarse_score", "coarse_all"},
    ("identify_many", "subject", False): {"group", "top_idx", "top_score", "subjects", "subject_score", "top_subject",
                                          "short_idx", "short_off"},
    ("identify_many", "subject", True): {"group", "top_idx", "top_score", "subjects", "subject_score", "top_subject",
                                         "short_subject", "coarse_subject_score", "coarse_all", "short_idx",
                                         "short_off"},
}
# dtype and length of the added keys: k ranks, Gs selected entries, M shortlisted entries or subjects, S ranked
# subjects (M when shortlisted), L entries in a subject-level query's lists
QUERY_KEY_FORMS = {
    "top_idx": (torch.int32, "k"), "top_score": (torch.float32, "k"), "top_subject": (torch.int64, "k"),
    "coarse_all": (torch.float32, "Gs"), "coarse_score": (torch.float32, "M"),
    "short_subject": (torch.int64, "M"), "coarse_subject_score": (torch.float32, "M"),
    "subjects": (torch.int64, "S"), "subject_score": (torch.float32, "S"), "short_off": (torch.int32, "S+1"),
}


def check_result_keys(r, call, by, shortlisted, run_keys=FORWARD_RUN_KEYS, **dims):
    """The exact key set of the result dict ``r`` of that query form (``run_keys``: those of FORWARD_RUN_KEYS
    this forward carries), and dtype, shape and device of every key the query layer added (``dims``: the
    lengths QUERY_KEY_FORMS names)."""
    added = QUERY_KEYS[(call, by, shortlisted)]
    want = FORWARD_KEYS | set(run_keys) | added
    assert set(run_keys) <= FORWARD_RUN_KEYS and set(r) == want, (call, by, shortlisted, sorted(set(r) ^ want))
    if "S" in dims:
        dims["S+1"] = dims["S"] + 1
    for key in sorted(added):
        if key == "group":
            assert isinstance(r[key], tuple) and len(r[key]) == 3
            continue
        dt, n = (torch.int32, "L" if by else "M") if key == "short_idx" else QUERY_KEY_FORMS[key]
        assert r[key].dtype == dt and tuple(r[key].shape) == (dims[n],) and r[key].device == DEV, (call, by, key)


MEASURED = {
    # case: (device_err, err32, device_err / err32, gate); scores 0.193-0.194 (flat), 0.168-0.288 (spread)
    "flat": (4.80e-08, 4.80e-08, 1.00, 3.84e-07),
    "spread": (5.74e-08, 1.48e-07, 0.39, 1.18e-06),
}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _net(sd, dtype="f32"):
    net = fpm.Net(regression=True, backbone=False, dtype=dtype)
    net.load_state_dict(sd)
    return net


@pytest.fixture(scope="module")
def sds():
    return state_dicts()


# ------------------------------------------------------------------------------ kernel vs float64
@pytest.mark.parametrize("name", ["flat", "spread"])
def test_coarse_kernel_vs_float64(name, sds):
    sd = sds[name]
    y, row_off, wg, probes = ragged_case(sd)
    idx = torch.tensor(list(range(len(ENTRY_NS))) + [2], dtype=torch.int32)      # one entry twice
    y_d, off_d, idx_d = y.to(DEV), row_off.to(DEV), idx.to(DEV)
    devs, refs, refs32, seen = [], [], [], set()
    for (yp, wp), n0 in zip(probes, PROBE_NS):
        coef = coefficients(wp, [wg[i] for i in idx.tolist()], sd)
        out = torch.full((idx.numel(),), float("nan"), device=DEV)
        ops.coarse_score(y_d, off_d, idx_d, yp.to(DEV), coef.to(DEV), out=out)
        devs.append(out.cpu().double())
        refs.append(ops.coarse_score(y, row_off, idx, yp, coef, dtype=torch.float64))
        refs32.append(ops.coarse_score(y, row_off, idx, yp, coef).double())
        assert float(out[2]) == float(out[-1])                                    # the entry used twice
        seen |= {(n0, ENTRY_NS[g]) for g in idx.tolist()}
    assert set(SHAPES) <= seen
    dev, ref, ref32 = torch.stack(devs), torch.stack(refs), torch.stack(refs32)
    assert bool(torch.isfinite(dev).all())
    err32 = float((ref32 - ref).abs().max())
    top = float(ref.abs().max())
    ulp = 2.0 ** (np.floor(np.log2(top)) - 23)
    gate = max(8 * ulp, 8 * err32)
    err = float((dev - ref).abs().max())
    print("MEASURE coarse %s err=%.3g err32=%.3g ratio=%.3g gate=%.3g scores=[%.3g, %.3g]"
          % (name, err, err32, err / err32, gate, float(ref.min()), float(ref.max())))
    assert err <= gate, "coarse %s: device error %.3g over the gate %.3g (err32 %.3g)" % (name, err, gate, err32)


# -------------------------------------------------------------------- planted-mate gallery (tests 2, 5, 6)
MATES = {7: 0, 19: 1, 38: 2}           # gallery entry -> probe
PROBE_N = (48, 33, 40)


def noisy_copy(g, seed):
    """A second impression of graph g: 3 keypoints dropped, the rest jittered by N(0, 1 px), features
    plus N(0, 0.01), Delaunay rebuilt, the same global feature."""
    rng = np.random.default_rng(seed)
    keep = np.sort(rng.permutation(g["n"])[:g["n"] - 3])
    P = (g["P"][keep].astype(np.float64) + rng.normal(0, 1.0, (keep.size, 2))).astype(np.float32).astype(np.float64)
    A = synth.delaunay_adjacency(P)
    ei, pseudo = synth.edges_from_adjacency(A, P)
    x = (g["x"][keep] + rng.normal(0, 0.01, g["x"][keep].shape)).astype(np.float32)
    return dict(P=P.astype(np.float32), A=A.astype(np.float32), edge_index=ei, pseudo=pseudo, x=x, w=g["w"].copy(),
                n=int(keep.size))


def planted():
    ns = np.random.default_rng(0).integers(24, 49, size=40)
    gal = [synth.make_graph(42, p, 1, int(n)) for p, n in enumerate(ns)]
    probes = [synth.make_graph(42, p, 0, n) for p, n in enumerate(PROBE_N)]
    for e, p in MATES.items():
        gal[e] = noisy_copy(probes[p], 1000 + e)
    return gal, probes


@pytest.fixture(scope="module")
def mates(sds):
    gal, probes = planted()
    net = _net(sds["spread"])
    index = net.enroll(gal, DEV, batch=16)
    return net, probes, gal, index


def test_coarse_composition_independence(mates):
    """An entry's score is the same bits alone, in the full launch and in a permuted selection walked
    in other chunks."""
    net, probes, gal, index = mates
    probe = probes[1]
    full = net.coarse_scores(probe, index)
    assert tuple(full.shape) == (1, len(gal)) and full.dtype == torch.float32 and full.device == index.device
    perm = torch.randperm(len(gal), generator=torch.Generator().manual_seed(3))
    mixed = gallery.coarse_scores(net, probe, index, select=perm, chunk=7)
    assert torch.equal(_bits(mixed[0]), _bits(full[0][perm.to(DEV)]))
    for e in (0, 7, 19, 39):
        alone = net.coarse_scores(probe, index, select=[e])
        assert torch.equal(_bits(alone[0]), _bits(full[0, e:e + 1])), e
    both = net.coarse_scores([probes[0], probe], index)
    assert torch.equal(_bits(both[1]), _bits(full[0]))


# -------------------------------------------------------------------------------------- rank_select
@pytest.mark.parametrize("P,G,k", [(2, 1000, 129), (3, 5000, 1024), (1, 100000, 1000), (2, 300, 7)])
def test_rank_select_device_equals_host(P, G, k):
    s = rank_scores(P, G, 100 + G)
    hi, hs = ops.rank_select(s, k)
    di, ds = ops.rank_select(s.to(DEV), k)
    assert di.dtype == torch.int32 and tuple(di.shape) == (P, k)
    assert torch.equal(di.cpu(), hi)
    assert torch.equal(_bits(ds.cpu()), _bits(hs))
    wide = torch.zeros(P, G + 9)                       # a strided view (row stride > G)
    wide[:, 4:4 + G] = s
    vi, vs = ops.rank_select(wide.to(DEV)[:, 4:4 + G], k)
    assert torch.equal(vi.cpu(), hi) and torch.equal(_bits(vs.cpu()), _bits(hs))
    if k <= 128:
        ti, ts = ops.rank_topk(s.to(DEV), k)
        assert torch.equal(ti, di) and torch.equal(_bits(ts), _bits(ds))


# -------------------------------------------------------------- shortlisted identify = selected identify
@pytest.fixture(scope="module", params=sorted(CASES))
def enrolled(request, sds):
    dtype, n_probe, ns, sc_mode = CASES[request.param]
    probe = synth.make_graph(40, 0, 0, n_probe)
    gal = [synth.make_graph(40, p, 1, n) for p, n in enumerate(ns)]
    net = _net(sds["flat"], dtype)
    index = net.enroll(gal, DEV, sc_mode=sc_mode, batch=4)
    return net, probe, gal, index


def test_shortlisted_identify_is_selected_identify(enrolled):
    net, probe, gal, index = enrolled
    res = net.identify(probe, index, topk=3, shortlist=3, chunks=2)
    assert res["short_idx"].dtype == torch.int32 and tuple(res["short_idx"].shape) == (3,)
    assert tuple(res["coarse_all"].shape) == (len(gal),)
    ref = net.identify(probe, index, topk=3, select=res["short_idx"], chunks=2)
    # chunks=2: no "Kp" / "coef"; the fp64 k chain when the probe and the shortlisted entries are within k_f64_nmax
    box = max([probe["n"]] + [gal[e]["n"] for e in res["short_idx"].tolist()])
    run_keys = {"ss64"} if box <= net.k_f64_nmax else set()
    check_result_keys(res, "identify", None, True, run_keys, k=3, M=3, Gs=len(gal))
    check_result_keys(ref, "identify", None, False, run_keys, k=3)
    for k in OUT_KEYS:
        assert torch.equal(res[k], ref[k]), k
    hi, hs = ops.rank_select(res["coarse_all"].cpu().view(1, -1), 3)
    assert torch.equal(res["short_idx"].cpu(), hi[0])
    assert torch.equal(_bits(res["coarse_score"].cpu()), _bits(hs[0]))
    assert torch.equal(_bits(res["coarse_all"]), _bits(net.coarse_scores(probe, index)[0]))
    # a selection, a list of probes, a shortlist over the selection's size (clamped)
    sel = [3, 0, 2]
    many = net.identify([probe], index, select=sel, shortlist=64, chunks=2)[0]
    assert sorted(many["short_idx"].tolist()) == sorted(sel) and tuple(many["coarse_all"].shape) == (3,)
    ref = net.identify(probe, index, select=many["short_idx"], chunks=2)
    for k in OUT_KEYS:
        assert torch.equal(many[k], ref[k]), k


# ------------------------------------------------------------------------------------ planted mate
def test_planted_mate_is_shortlisted(mates, sds):
    net, probes, gal, index = mates
    wp = net.packed(DEV)
    y, off = index.y.cpu(), index.row_off_host
    idx = torch.arange(len(gal), dtype=torch.int32)
    res = net.identify(probes, index, topk=4, shortlist=4)
    for p, probe in enumerate(probes):
        # the CPU ranking, float64, on the device's own operands
        yp = net._probe_rows(wp, gallery._ProbeSide(probe, index)).cpu()
        coef = coefficients(probe["w"], [g["w"] for g in gal], sds["spread"])
        coef_d = torch.empty(len(gal), 768, device=DEV)
        w0 = torch.from_numpy(probe["w"]).to(DEV).view(1, -1).expand(len(gal), -1).contiguous()
        ops.coef_tanh(ops.global_weights(w0, index.w), wp["aff_wT"], wp["aff_b"], coef_d)
        assert float((coef_d.cpu() - coef).abs().max()) < 1e-5
        sc = ops.coarse_score(y, off, idx, yp, coef_d.cpu(), dtype=torch.float64)
        order = torch.argsort(sc, descending=True, stable=True)
        mate = [e for e, q in MATES.items() if q == p][0]
        top = sc[order]
        print("MEASURE mate probe %d: top5 %s at %s" % (p, [round(float(v), 6) for v in top[:5]], order[:5].tolist()))
        # the precondition, on the CPU ranking: mate first by more than 1.0, ranks 1..5 well apart
        assert int(order[0]) == mate and float(top[0] - top[1]) > 1.0
        assert float((top[:4] - top[1:5]).min()) > 1e-5
        assert res[p]["short_idx"].tolist() == order[:4].tolist()
        assert int(res[p]["short_idx"][0]) == mate
        assert float((res[p]["coarse_all"].cpu().double() - sc).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------- refusals
def test_refusals(mates, sds):
    net, probes, gal, index = mates
    probe = probes[0]
    for m in (0, 2000):
        with pytest.raises(_lib.FpmError, match="shortlist"):
            net.identify(probe, index, shortlist=m)
    big = synth.make_graph(42, 0, 0, 130)
    with pytest.raises(_lib.FpmError, match="COARSE_NMAX"):
        net.identify(big, index, shortlist=2)
    with pytest.raises(_lib.FpmError, match="COARSE_NMAX"):
        net.coarse_scores(big, index)
    index_big = net.enroll([gal[0], synth.make_graph(42, 1, 1, 130)], DEV)
    with pytest.raises(_lib.FpmError, match="COARSE_NMAX"):
        net.identify(probe, index_big, shortlist=1)
    assert net.identify(probe, index_big, shortlist=1, select=[0])["short_idx"].tolist() == [0]
    net.train()
    try:
        for call in (lambda: net.identify(probe, index, shortlist=2), lambda: net.coarse_scores(probe, index)):
            with pytest.raises(_lib.FpmError, match="inference only"):
                call()
    finally:
        net.eval()
    other = _net(params.init_params(8))
    for call in (lambda: other.identify(probe, index, shortlist=2), lambda: other.coarse_scores(probe, index)):
        with pytest.raises(_lib.FpmError, match="other SplineConv weights"):
            call()
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
        (dict(), "COARSE_NMAX"),                                   # entry 1 has 130 keypoints
        (dict(idx=idx[:1].repeat(2), yp=torch.zeros(129, 768, device=DEV)), "COARSE_NMAX"),
        (dict(idx=idx.cpu()), "is on"),
    ]
    for kw, msg in bad:
        a = dict(idx=idx, yp=yp)
        a.update(kw)
        with pytest.raises(_lib.FpmError, match=msg):
            ops.coarse_score(yb, ob, a["idx"], a["yp"], coef, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    s = torch.zeros(2, 2000, device=DEV)
    for k in (0, 2001, 1025):
        with pytest.raises(_lib.FpmError, match="rank_select: k"):
            ops.rank_select(s, k)


# ------------------------------------------------------------------------------------------- C-ABI
def test_c_abi_entry_points(mates):
    net, probes, gal, index = mates
    lib = _lib.load()
    P = ctypes.c_void_p
    st = P(torch.cuda.current_stream(DEV).cuda_stream)
    wp = net.packed(DEV)
    probe = probes[2]
    yp = net._probe_rows(wp, gallery._ProbeSide(probe, index))
    B = 5
    idx = torch.tensor([4, 38, 0, 38, 11], dtype=torch.int32, device=DEV)
    coef = torch.empty(B, 768, device=DEV)
    w0 = torch.from_numpy(probe["w"]).to(DEV).view(1, -1).expand(B, -1).contiguous()
    ops.coef_tanh(ops.global_weights(w0, index.w[idx.long()]), wp["aff_wT"], wp["aff_b"], coef)
    out = torch.full((B,), float("nan"), device=DEV)
    rc = lib.fpm_coarse_score(P(index.y.data_ptr()), P(index.row_off.data_ptr()), P(idx.data_ptr()), index.G, B,
                              P(yp.data_ptr()), int(yp.shape[0]), P(coef.data_ptr()), 10, 0.01, P(out.data_ptr()), st)
    assert rc == 0
    ref = net.coarse_scores(probe, index, select=idx.cpu())
    assert torch.equal(_bits(out), _bits(ref[0]))
    rc = lib.fpm_coarse_score(P(index.y.data_ptr()), P(index.row_off.data_ptr()), P(idx.data_ptr()), index.G, B,
                              P(yp.data_ptr()), 129, P(coef.data_ptr()), 10, 0.01, P(out.data_ptr()), st)
    assert rc != 0 and b"COARSE_NMAX" in lib.fpm_last_error()

    s = rank_scores(2, 4000, 9).to(DEV)
    k = 300
    ti = torch.empty(2, k, dtype=torch.int32, device=DEV)
    ts = torch.empty(2, k, device=DEV)
    wsb = int(lib.fpm_rank_select_ws_bytes(2))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    rc = lib.fpm_rank_select(P(s.data_ptr()), 4000, 2, 4000, k, P(ti.data_ptr()), P(ts.data_ptr()), P(ws.data_ptr()),
                             wsb, st)
    assert rc == 0
    hi, hs = ops.rank_select(s.cpu(), k)
    assert torch.equal(ti.cpu(), hi) and torch.equal(_bits(ts.cpu()), _bits(hs))
    rc = lib.fpm_rank_select(P(s.data_ptr()), 4000, 2, 4000, 1025, P(ti.data_ptr()), P(ts.data_ptr()),
                             P(ws.data_ptr()), wsb, st)
    assert rc != 0 and b"rank_select: k" in lib.fpm_last_error()
    rc = lib.fpm_rank_select(P(s.data_ptr()), 4000, 2, 4000, k, P(ti.data_ptr()), P(ts.data_ptr()), P(ws.data_ptr()),
                             wsb - 8, st)
    assert rc != 0 and b"workspace" in lib.fpm_last_error()

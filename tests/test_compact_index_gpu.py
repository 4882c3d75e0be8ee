"""Compact gallery index on the GPU: the three coarse kernels on bf16 index rows against the same
kernels on the fp32 rows (bit for bit: the operands are identical by construction, no tolerance),
``ops.rows_fetch`` from pinned host memory and from the device, the three index layouts against each
other through ``coarse_scores`` and ``identify`` on every coarse route, ``save`` / ``load`` of a
"bf16+host" index, the refusals and the C-ABI of the ``*_rows16`` entry points."""
import ctypes

import pytest
import torch

from fpm import _lib, gallery, ops, params, synth
from fpm.gallery import GalleryIndex
from test_coarse_stream_cpu import STREAM_SHAPES
from test_coarse_wide_cpu import WIDE_SHAPES, synthetic_case
from test_compact_index_cpu import FETCH_NS, fetch_case, out_offsets
from test_shortlist_cpu import ENTRY_NS, PROBE_NS, SHAPES, coefficients, ragged_case, state_dicts
from test_shortlist_gpu import MATES, OUT_KEYS, _bits, _net, planted

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LAYOUTS = ("f32", "f32+bf16", "bf16+host")
KEYS = OUT_KEYS + ("short_idx", "coarse_score", "coarse_all")


@pytest.fixture(scope="module")
def sds():
    return state_dicts()


def _bits16(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------- kernels, bit for bit
def _fused_pairs(sd):
    """``ragged_case`` as ``test_coarse_kernel_vs_float64`` walks it: SHAPES, one entry twice."""
    y, row_off, wg, probes = ragged_case(sd)
    idx = torch.tensor(list(range(len(ENTRY_NS))) + [2], dtype=torch.int32)
    out = [(n0, yp, idx, coefficients(wp, [wg[i] for i in idx.tolist()], sd)) for (yp, wp), n0 in zip(probes, PROBE_NS)]
    return y, row_off, out, ENTRY_NS


def _synthetic_pairs(shapes):
    y, row_off, probes = synthetic_case("spread", shapes)
    return y, row_off, probes, sorted({b for _, b in shapes})


@pytest.mark.parametrize("kernel", ["fused", "wide", "stream"])
def test_kernel_on_bf16_rows_bit_for_bit(kernel, sds):
    """The kernel's own shape set (every tile edge, the transpose, the dummy rows); each probe's
    index list names one entry twice."""
    op, shapes = {"fused": (ops.coarse_score, SHAPES), "wide": (ops.coarse_score_wide, WIDE_SHAPES),
                  "stream": (ops.coarse_score_stream, STREAM_SHAPES)}[kernel]
    y, row_off, probes, entry_ns = _fused_pairs(sds["spread"]) if kernel == "fused" else _synthetic_pairs(shapes)
    y_d, off_d = y.to(DEV), row_off.to(DEV)
    y16 = ops.cast_bf16(y_d)
    assert y16.dtype == torch.bfloat16 and torch.equal(_bits16(y16), _bits16(y_d.to(torch.bfloat16)))
    seen = set()
    for n0, yp, idx, coef in probes:
        a = (off_d, idx.to(DEV), yp.to(DEV), coef.to(DEV))
        ref = torch.full((idx.numel(),), float("nan"), device=DEV)
        got = torch.full((idx.numel(),), float("nan"), device=DEV)
        op(y_d, *a, out=ref, idx_host=idx, row_off_host=row_off)
        op(y16, *a, out=got, idx_host=idx, row_off_host=row_off)
        assert bool(torch.isfinite(got).all()), n0
        assert torch.equal(_bits(got), _bits(ref)), (n0, got.tolist(), ref.tolist())
        dup = idx.tolist().index(int(idx[-1]))
        assert dup < idx.numel() - 1 and int(_bits(got)[dup]) == int(_bits(got)[-1])
        seen |= {(n0, entry_ns[g]) for g in idx.tolist()}
    assert set(shapes) <= seen


# --------------------------------------------------------------------------------------- rows_fetch
@pytest.mark.parametrize("source", ["pinned", "device"])
def test_rows_fetch(source):
    y, row_off = fetch_case(FETCH_NS + (600,))
    src = torch.empty(y.shape, pin_memory=True).copy_(y) if source == "pinned" else y.to(DEV)
    assert src.is_pinned() or src.is_cuda
    off_d = row_off.to(DEV)
    for sel in ([4, 0, 2, 0, 3, 1, 5], [3], [0], [5]):
        idx = torch.tensor(sel, dtype=torch.int32)
        off = out_offsets(row_off, idx)
        total = int(off[-1])
        out = torch.full((total + 3, 768), float("nan"), device=DEV)
        ops.rows_fetch(src, off_d, idx.to(DEV), out, off.to(DEV), idx_host=idx, row_off_host=row_off,
                       out_off_host=off)
        want = torch.cat([y[int(row_off[g]):int(row_off[g + 1])] for g in sel])
        assert torch.equal(out[:total].cpu(), want), sel
        assert bool(torch.isnan(out[total:]).all()), sel            # nothing past the selection is written
    with pytest.raises(_lib.FpmError, match="must be pinned"):
        ops.rows_fetch(y, off_d, idx.to(DEV), out, off.to(DEV), idx_host=idx, row_off_host=row_off)
    with pytest.raises(_lib.FpmError, match="out_off must rise"):                 # checked from the device copy
        ops.rows_fetch(src, off_d, idx.to(DEV), out, (off + 1).to(DEV), idx_host=idx, row_off_host=row_off)
    with pytest.raises(_lib.FpmError, match="out holds"):
        ops.rows_fetch(src, off_d, idx.to(DEV), out[:total - 1], off.to(DEV), idx_host=idx, row_off_host=row_off)


# ------------------------------------------------------------------------------ layouts agree, fused
@pytest.fixture(scope="module", params=["f32", "bf16"])
def enrolled(request, sds):
    """The planted-mate gallery of ``test_shortlist_gpu`` enrolled once per layout by one net."""
    gal, probes = planted()
    net = _net(sds["spread"], request.param)
    return net, probes, gal, {lay: net.enroll(gal, DEV, batch=16, layout=lay) for lay in LAYOUTS}


def _same(a, b, keys=KEYS):
    for k in keys:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    for k in ("coarse_score", "coarse_all"):
        if k in keys:
            assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_layouts_hold_what_they_say(enrolled):
    net, probes, gal, idx = enrolled
    f32, both, host = (idx[lay] for lay in LAYOUTS)
    rows = sum(g["n"] for g in gal)
    assert f32.y16 is None and f32.y.is_cuda and f32.host_nbytes() == 0
    assert both.y.is_cuda and both.y16.is_cuda and both.nbytes() == f32.nbytes() + rows * 768 * 2
    assert host.y16.is_cuda and not host.y.is_cuda and host.y.is_pinned() and host.device == DEV
    assert host.nbytes() == f32.nbytes() - rows * 768 * 2 and host.host_nbytes() == rows * 768 * 4
    for other in (both, host):
        assert torch.equal(_bits(other.y.cpu()), _bits(f32.y.cpu()))
        assert torch.equal(_bits16(other.y16), _bits16(f32.y.to(torch.bfloat16)))


def test_layouts_agree_fused(enrolled):
    net, probes, gal, idx = enrolled
    ref_c = net.coarse_scores(probes, idx["f32"])
    ref_1 = net.identify(probes[1], idx["f32"], shortlist=8, topk=5)
    ref_n = net.identify(probes, idx["f32"], shortlist=8, topk=5)
    assert tuple(ref_1["short_idx"].shape) == (8,) and tuple(ref_1["top_idx"].shape) == (5,)
    for lay in LAYOUTS[1:]:
        assert torch.equal(_bits(net.coarse_scores(probes, idx[lay])), _bits(ref_c)), lay
        _same(net.identify(probes[1], idx[lay], shortlist=8, topk=5), ref_1)
        res = net.identify(probes, idx[lay], shortlist=8, topk=5)
        assert len(res) == len(probes)
        for a, b in zip(res, ref_n):
            _same(a, b)
        if net.dtype_mode == "f32":             # test_planted_mate_is_shortlisted's precondition holds there
            for p in range(len(probes)):
                mate = [e for e, q in MATES.items() if q == p][0]
                assert int(res[p]["short_idx"][0]) == mate, (lay, p)


def test_without_a_shortlist(enrolled, monkeypatch):
    net, probes, gal, idx = enrolled
    ref = net.identify(probes[0], idx["f32"], select=[5, 2, 7])
    for lay in LAYOUTS[1:]:
        res = net.identify(probes[0], idx[lay], select=[5, 2, 7])
        _same(res, ref, OUT_KEYS)
        assert sorted(res["top_idx"].tolist()) == [2, 5, 7]
    # a selection whose rows exceed the staging cap is refused; a shortlist within it is served
    rows = [int(g["n"]) for g in gal]
    monkeypatch.setattr(gallery, "FETCH_MAX_BYTES", 8 * max(rows) * 3072)
    with pytest.raises(_lib.FpmError, match="shortlist="):
        net.identify(probes[0], idx["bf16+host"])
    _same(net.identify(probes[1], idx["bf16+host"], shortlist=8, topk=5),
          net.identify(probes[1], idx["f32"], shortlist=8, topk=5))
    assert net.identify(probes[0], idx["f32+bf16"])["top_idx"].numel() == 10      # rows on the device: no cap


def test_save_load_on_the_device(enrolled, tmp_path):
    net, probes, gal, idx = enrolled
    path = str(tmp_path / "compact.pt")
    idx["bf16+host"].save(path)
    back = GalleryIndex.load(path, DEV)
    assert back.layout == "bf16+host" and back.device == DEV
    assert back.y.is_pinned() and not back.y.is_cuda and back.y16.is_cuda
    _same(net.identify(probes[2], back, shortlist=8, topk=5), net.identify(probes[2], idx["f32"], shortlist=8, topk=5))


def test_other_weights_refused_for_every_layout(enrolled):
    net, probes, gal, idx = enrolled
    other = _net(params.init_params(8), net.dtype_mode)
    for lay in LAYOUTS:
        for call in (lambda: other.identify(probes[0], idx[lay], shortlist=2), lambda: other.identify(probes[0], idx[lay]),
                     lambda: other.coarse_scores(probes[0], idx[lay])):
            with pytest.raises(_lib.FpmError, match="other SplineConv weights"):
                call()


# ------------------------------------------------------------------------ layouts agree, mixed routes
MIXED_N = (24, 48, 128, 129, 200, 256, 257, 300)
MIXED_PROBES = (40, 131, 259)


def test_layouts_agree_mixed_routes(sds):
    gal = [synth.make_graph(42, p, 1, n) for p, n in enumerate(MIXED_N)]
    probes = [synth.make_graph(42, p, 0, n) for p, n in enumerate(MIXED_PROBES)]
    net = _net(sds["spread"])
    f32 = net.enroll(gal, DEV, batch=4, layout="f32")
    host = net.enroll(gal, DEV, batch=4, layout="bf16+host")
    # the first probe meets all three kernels in one chunk, the second two, the third the stream kernel alone
    assert [sorted(set(gallery.coarse_routes(n0, f32.n, "any").tolist())) for n0 in MIXED_PROBES] \
        == [[0, 1, 2], [1, 2], [2]]
    ref = net.identify(probes, f32, shortlist=3, topk=3, coarse="any")
    res = net.identify(probes, host, shortlist=3, topk=3, coarse="any")
    for a, b in zip(res, ref):
        assert bool(torch.isfinite(a["coarse_all"]).all())
        _same(a, b)


# ------------------------------------------------------------------------------------------- C-ABI
def test_rows16_c_abi_entry_points(enrolled):
    net, probes, gal, idx = enrolled
    index = idx["f32+bf16"]
    lib = _lib.load()
    P = ctypes.c_void_p
    st = P(torch.cuda.current_stream(DEV).cuda_stream)
    wp = net.packed(DEV)
    probe = probes[2]
    yp = net._probe_rows(wp, gallery._ProbeSide(probe, index))
    B = 5
    sel = torch.tensor([4, 38, 0, 38, 11], dtype=torch.int32, device=DEV)
    coef = torch.empty(B, 768, device=DEV)
    w0 = torch.from_numpy(probe["w"]).to(DEV).view(1, -1).expand(B, -1).contiguous()
    ops.coef_tanh(ops.global_weights(w0, index.w[sel.long()]), wp["aff_wT"], wp["aff_b"], coef)
    n0 = int(yp.shape[0])
    wsb = max(int(lib.fpm_coarse_score_wide_ws_bytes(B)), int(lib.fpm_coarse_score_stream_ws_bytes(B, n0, 48)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    head = (P(index.row_off.data_ptr()), P(sel.data_ptr()), index.G, B, P(yp.data_ptr()))
    cases = [(lib.fpm_coarse_score_rows16, lib.fpm_coarse_score, (), b"COARSE_NMAX", 129),
             (lib.fpm_coarse_score_wide_rows16, lib.fpm_coarse_score_wide, (P(ws.data_ptr()), wsb),
              b"COARSE_WIDE_NMAX", 257),
             (lib.fpm_coarse_score_stream_rows16, lib.fpm_coarse_score_stream, (P(ws.data_ptr()), wsb),
              b"COARSE_STREAM_NMAX", 601)]
    for fn16, fn32, wsa, bound, over in cases:
        tail = lambda out: (P(coef.data_ptr()), 10, 0.01, P(out.data_ptr())) + wsa + (st,)
        got = torch.full((B,), float("nan"), device=DEV)
        ref = torch.full((B,), float("nan"), device=DEV)
        assert fn16(P(index.y16.data_ptr()), *head, n0, *tail(got)) == 0
        assert fn32(P(index.y.data_ptr()), *head, n0, *tail(ref)) == 0
        assert bool(torch.isfinite(got).all()) and torch.equal(_bits(got), _bits(ref))
        untouched = torch.full((B,), float("nan"), device=DEV)
        rc = fn16(P(index.y16.data_ptr()), *head, over, *tail(untouched))
        assert rc != 0 and bound in lib.fpm_last_error()
        rc = fn16(P(0), *head, n0, *tail(untouched))
        assert rc != 0 and b"are required" in lib.fpm_last_error()
        rc = fn16(P(index.y16.data_ptr()), P(0), *head[1:], n0, *tail(untouched))
        assert rc != 0 and b"are required" in lib.fpm_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isnan(untouched).all())

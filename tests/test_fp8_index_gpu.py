"""The fp8 index on the GPU: ``fpm_rows_quant8`` against its host statement (bytes and scales, bit for bit), each
of the six ``_rows8`` coarse entry points against its ``_rows16`` sibling on the dequantised rows (bit for bit, over
that kernel's own shape set), ``fpm_rows_move8`` against the copy's statement, and the "fp8+host" layout through
enrolment, the queries, the mutable index and shards.

Bit identity is the whole gate here: the quantisation is defined in torch, the dequantised operand is exact in
bf16, and everything after the coarse score is the other layouts' code."""
import pytest
import torch

from fpm import _lib, gallery, ops, params
from fpm.gallery import GalleryIndex
from fpm.sharded_gallery import ShardedGallery
from test_coarse_stream_cpu import STREAM_SHAPES
from test_coarse_wide_cpu import WIDE_SHAPES
from test_enroll_keypoints_gpu import CASES, DEV, _export, _keypoint_set, _net
from test_fp8_index_cpu import FP8, _u8, pair_list, same_fields8, scaled_case, special_rows
from test_mutable_index_gpu import APPENDED, SUBJECTS, same_results
from test_sharded_gallery_gpu import _check_against
from test_shortlist_cpu import SHAPES
from test_shortlist_gpu import OUT_KEYS

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------- rows_quant8
@pytest.mark.parametrize("rows", [1, 3, 65, 257])
def test_rows_quant8_device_is_the_host_statement(rows):
    """Four rows per workgroup: the special rows first, last and across the boundary of workgroups 0 / 1 (and
    15 / 16, 63 / 64), seeded rows of many scales between; guard rows after the outputs keep their fill."""
    sp, names = special_rows()
    g = torch.Generator().manual_seed(rows)
    y = torch.randn(rows, 768, generator=g) * torch.ldexp(torch.ones(rows), torch.arange(rows) % 61 - 30)[:, None]
    ns = sp.shape[0]
    for at in (0, 2, 62, 254, rows - ns):                    # rows 2 .. 15: workgroups 0 to 3; 62 ..: 15 to 18
        if 0 <= at and at + ns <= rows:
            y[at:at + ns] = sp
    if rows < ns:
        y[:] = sp[[names["ties"], names["subnormal"], names["1e-38"]][:rows]]
    w8, ws = ops.rows_quant8(y)
    guard = 3
    y8 = torch.full((rows + guard, 768), 0x55, dtype=torch.uint8, device=DEV).view(FP8)
    s8 = torch.full((rows + guard,), -7.0, device=DEV)
    got = ops.rows_quant8(y.to(DEV), y8[:rows], s8[:rows])
    torch.cuda.synchronize()
    assert got[0].data_ptr() == y8.data_ptr() and got[1].data_ptr() == s8.data_ptr()
    assert torch.equal(_bits(s8[:rows].cpu()), _bits(ws))
    bad = (_u8(y8[:rows].cpu()) != _u8(w8)).nonzero()
    assert bad.numel() == 0, (bad[:5].tolist(), y[bad[0, 0], bad[0, 1]].item())
    assert bool((_u8(y8[rows:]) == 0x55).all()) and bool((s8[rows:] == -7.0).all())
    # allocated outputs; rows = 0 launches nothing
    a8, as_ = ops.rows_quant8(y.to(DEV))
    assert a8.dtype == FP8 and torch.equal(_u8(a8.cpu()), _u8(w8)) and torch.equal(as_.cpu(), ws)
    e8, es = ops.rows_quant8(torch.zeros(0, 768, device=DEV))
    assert tuple(e8.shape) == (0, 768) and tuple(es.shape) == (0,)


def test_rows_quant8_device_refusals_launch_nothing():
    y = torch.ones(4, 768, device=DEV)
    y8 = torch.full((4, 768), 0x55, dtype=torch.uint8, device=DEV).view(FP8)
    s8 = torch.full((4,), -7.0, device=DEV)
    R = lambda m: pytest.raises(_lib.FpmError, match=m)
    with R("y8 is on"):
        ops.rows_quant8(y, y8.cpu(), s8)
    with R("s8 is on"):
        ops.rows_quant8(y, y8, s8.cpu())
    with R("16-byte aligned"):
        ops.rows_quant8(torch.ones(4 * 768 + 1, device=DEV)[1:].view(4, 768), y8, s8)
    with R("y8 must be contiguous float8_e4m3fn rows"):
        ops.rows_quant8(y, y8[:3], s8)
    torch.cuda.synchronize()
    assert bool((_u8(y8) == 0x55).all()) and bool((s8 == -7.0).all())


# ------------------------------------------------------------------------ the six _rows8 entry points
KERNELS = {"fused": (SHAPES, ops.coarse_score), "wide": (WIDE_SHAPES, ops.coarse_score_wide),
           "stream": (STREAM_SHAPES, ops.coarse_score_stream)}
_CASES = {}


def _case(kernel):
    if kernel not in _CASES:
        _CASES[kernel] = scaled_case(KERNELS[kernel][0])
    return _CASES[kernel]


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_rows8_entry_points_equal_rows16_on_the_dequantised_rows(kernel):
    """One probe: the full launch on fp8 rows is the bf16 launch's bits, and a score alone is its score in the
    full launch.  The pair list: every pair of the case in a permuted order, the bf16 pair list's bits and the
    one-probe launches'."""
    shapes, op = KERNELS[kernel]
    y, row_off, probes, y8, s8, y16 = _case(kernel)
    y8_d, s8_d, y16_d, off_d = y8.to(DEV), s8.to(DEV), y16.to(DEV), row_off.to(DEV)
    seen, one = set(), {}
    for q, (n0, yp, idx, coef) in enumerate(probes):
        yp_d, idx_d, coef_d = yp.to(DEV), idx.to(DEV), coef.to(DEV)
        got = torch.full((idx.numel(),), float("nan"), device=DEV)
        op(y8_d, off_d, idx_d, yp_d, coef_d, out=got, row_scale=s8_d, idx_host=idx, row_off_host=row_off)
        want = op(y16_d, off_d, idx_d, yp_d, coef_d, idx_host=idx, row_off_host=row_off)
        assert bool(torch.isfinite(got).all()) and torch.equal(_bits(got), _bits(want)), n0
        for b in (0, idx.numel() // 2):
            alone = op(y8_d, off_d, idx_d[b:b + 1].contiguous(), yp_d, coef_d[b:b + 1].contiguous(), row_scale=s8_d)
            assert torch.equal(_bits(alone), _bits(got[b:b + 1])), (n0, b)
        one[q] = got
        seen |= {(n0, int(row_off[e + 1] - row_off[e])) for e in idx.tolist()}
    assert set(shapes) <= seen
    yq, qrow_off, qidx, gidx, coef, pairs = pair_list(probes)
    args = (off_d, gidx.to(DEV), yq.to(DEV), qrow_off.to(DEV), qidx.to(DEV), coef.to(DEV))
    host = dict(kernel=kernel, gidx_host=gidx, qidx_host=qidx, row_off_host=row_off, qrow_off_host=qrow_off)
    got = ops.coarse_pairs(y8_d, *args, row_scale=s8_d, **host)
    want = ops.coarse_pairs(y16_d, *args, **host)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(got), _bits(torch.stack([one[q][b] for q, b in pairs])))


def test_rows8_c_abi_refusals_launch_nothing():
    """A missing scale array is refused by name; a violating pair reads nothing and gets NaN."""
    import ctypes
    lib = _lib.load()
    P = ctypes.c_void_p
    y, row_off, probes, y8, s8, _ = _case("fused")
    n0, yp, idx, coef = probes[-1]
    st = P(torch.cuda.current_stream(DEV).cuda_stream)
    y8_d, s8_d, off_d, yp_d, coef_d = y8.to(DEV), s8.to(DEV), row_off.to(DEV), yp.to(DEV), coef.to(DEV)
    G, B = int(row_off.numel()) - 1, int(idx.numel())
    out = torch.full((B,), 5.0, device=DEV)
    a = lambda t: P(t.data_ptr())
    rc = lib.fpm_coarse_score_rows8(a(y8_d), P(0), a(off_d), a(idx.to(DEV)), G, B, a(yp_d), n0, a(coef_d), 10, 0.01,
                                    a(out), st)
    assert rc != 0 and b"are required" in lib.fpm_last_error()
    rc = lib.fpm_coarse_score_rows8(a(y8_d), a(s8_d), a(off_d), a(idx.to(DEV)), G, B, a(yp_d), 129, a(coef_d), 10, 0.01,
                                    a(out), st)
    assert rc != 0 and b"COARSE_NMAX" in lib.fpm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    bad = idx.clone()
    bad[1] = G                                               # outside [0, G): nothing of it is read
    rc = lib.fpm_coarse_score_rows8(a(y8_d), a(s8_d), a(off_d), a(bad.to(DEV)), G, B, a(yp_d), n0, a(coef_d), 10, 0.01,
                                    a(out), st)
    assert rc == 0
    ref = ops.coarse_score(y8_d, off_d, idx.to(DEV), yp_d, coef_d, row_scale=s8_d)
    keep = torch.arange(B) != 1
    assert bool(torch.isnan(out[1])) and torch.equal(_bits(out.cpu()[keep]), _bits(ref.cpu()[keep]))


# ------------------------------------------------------------------------------------- rows_move8
def test_rows_move8_bits():
    """The segment cases of the fp32 / bf16 copy (empty and adjacent segments, one row, both sides of the 16-row
    band) to another buffer, inside one buffer through a stage where a destination meets its source, and directly
    where it does not; rows and scales outside the destinations keep their fill."""
    from test_mutable_index_cpu import move_case, move_statement
    src, so, do, cnt, rows = move_case()
    sp, _ = special_rows()
    src = torch.nan_to_num(src, nan=3.0).clamp(-1e30, 1e30)      # finite rows: the quantisation is defined on them
    src[:sp.shape[0]] = sp
    s8, ss = ops.rows_quant8(src * torch.ldexp(torch.ones(src.shape[0]), torch.arange(src.shape[0]) % 40 - 20)[:, None])
    b8, bs = _u8(s8), ss.clone()
    s8_d, ss_d = s8.to(DEV), ss.to(DEV)
    d8 = torch.full((rows + 3, 768), 0x55, dtype=torch.uint8, device=DEV).view(FP8)
    ds = torch.full((rows + 3,), -7.0, device=DEV)
    got = ops.rows_move(so.to(DEV), do.to(DEV), cnt.to(DEV), src8=s8_d, dst8=d8, srcs=ss_d, dsts=ds, src_off_host=so,
                        dst_off_host=do, cnt_host=cnt)
    torch.cuda.synchronize()
    assert got[0] is d8 and got[1] is ds
    want8 = move_statement(b8, so, do, cnt, torch.full((rows + 3, 768), 0x55, dtype=torch.uint8))
    wants = move_statement(bs, so, do, cnt, torch.full((rows + 3,), -7.0))
    assert torch.equal(_u8(d8.cpu()), want8) and torch.equal(_bits(ds.cpu()), _bits(wants))
    so2 = torch.tensor([3, 30, 50, 90], dtype=torch.int64)
    cn2 = torch.tensor([17, 16, 33, 1], dtype=torch.int64)
    do2 = torch.cat([torch.zeros(1, dtype=torch.int64), cn2.cumsum(0)[:-1]])
    with pytest.raises(_lib.FpmError, match="a destination range meets a source range"):
        ops.rows_move(so2.to(DEV), do2.to(DEV), cn2.to(DEV), src8=s8_d, dst8=s8_d, srcs=ss_d, dsts=ss_d)
    g8, gs = torch.empty(67, 768, device=DEV, dtype=FP8), torch.empty(67, device=DEV)
    ops.rows_move(so2.to(DEV), do2.to(DEV), cn2.to(DEV), src8=s8_d, dst8=g8, srcs=ss_d, dsts=gs)
    ops.rows_move(do2.to(DEV), do2.to(DEV), cn2.to(DEV), src8=g8, dst8=s8_d, srcs=gs, dsts=ss_d)
    far, near, cn3 = torch.tensor([80, 90]), torch.tensor([67, 74]), torch.tensor([7, 6])    # 80 .. 96 to 67 .. 80
    ops.rows_move(far.to(DEV), near.to(DEV), cn3.to(DEV), src8=s8_d, dst8=s8_d, srcs=ss_d, dsts=ss_d)
    torch.cuda.synchronize()
    for got, b in ((_u8(s8_d.cpu()), b8), (ss_d.cpu(), bs)):
        want = move_statement(b.clone(), so2, do2, cn2, b.clone())
        want = move_statement(want.clone(), far, near, cn3, want)
        assert torch.equal(_u8(got), _u8(want))


# ------------------------------------------------------------------------------------- the index
@pytest.fixture(scope="module", params=["f32ops-f32", "bf16ops"])
def world(request):
    dtype, n_probe, ns, sc_mode = CASES[request.param]
    net = _net(params.init_params(7), dtype)
    A, B = _keypoint_set(ns, 11), _keypoint_set(APPENDED[request.param], 21)
    dA, dB = _export(*A), _export(*B)
    sA, sB = SUBJECTS[len(dA)], SUBJECTS[len(dB)]
    probe = _export(*_keypoint_set([n_probe], 12))[0]
    pdicts = _export(*_keypoint_set([max(ns)] * 3, 13))      # one box for every probe and the whole gallery
    kw = dict(sc_mode=sc_mode, batch=4)
    index = {lay: net.enroll(dA + dB, DEV, layout=lay, subjects=sA + sB, **kw) for lay in ("f32", "bf16+host", "fp8+host")}
    pset = net.enroll(pdicts, DEV, sc_mode=sc_mode, batch=2)
    i8 = index["fp8+host"]
    hand = GalleryIndex(i8.y, i8.row_off, i8.n, i8.src, i8.dst, i8.pseudo, i8.edge_off, i8.w, i8.P, i8.sc_mode,
                        i8._pack_gen, i8.weights_id, y16=ops.rows_dequant8(i8.y8, i8.s8), layout="bf16+host",
                        subject=i8.subject)
    return dict(net=net, A=A, B=B, dA=dA, dB=dB, sA=sA, sB=sB, probe=probe, pdicts=pdicts, pset=pset, index=index,
                hand=hand, kw=kw)


def test_enrolments_give_the_quantised_rows(world):
    net, i8, i16 = world["net"], world["index"]["fp8+host"], world["index"]["bf16+host"]
    assert i8.layout == "fp8+host" and i8.y16 is None and i8.y8.dtype == FP8 and i8.y8.is_cuda and i8.s8.is_cuda
    assert not i8.y.is_cuda and i8.y.is_pinned() and torch.equal(_bits(i8.y), _bits(i16.y))
    w8, ws = ops.rows_quant8(i8.y.clone())                                       # the host statement
    assert torch.equal(_u8(i8.y8.cpu()), _u8(w8)) and torch.equal(_bits(i8.s8.cpu()), _bits(ws))
    assert int(torch.unique(ws).numel()) > 1
    R_ = int(i8.y.shape[0])
    assert i16.nbytes() - i8.nbytes() == R_ * (1536 - 772) and i8.host_nbytes() == R_ * 3072
    P, n, x, w = (torch.cat([a, b]) if a.shape[1:] == b.shape[1:] else None for a, b in zip(world["A"], world["B"]))
    if P is not None:                                                            # the two sets share nmax
        kp = net.enroll_keypoints(P.to(DEV), n, x.to(DEV), w.to(DEV), layout="fp8+host",
                                  subjects=world["sA"] + world["sB"], **world["kw"])
        same_fields8(kp, i8, "keypoints")
    kpA = net.enroll_keypoints(*[t.to(DEV) for t in world["A"]], layout="fp8+host", subjects=world["sA"], **world["kw"])
    same_fields8(kpA, net.enroll(world["dA"], DEV, layout="fp8+host", subjects=world["sA"], **world["kw"]), "A")
    same_fields8(kpA, i8.slice(torch.arange(len(world["dA"]))), "A of AB")


def test_enroll_images_gives_the_quantised_rows():
    """The image route on captured backbone features (MIOpen's are not reproducible call to call): the index
    equals ``enroll_keypoints`` on those features, every field."""
    import fpm
    net = fpm.Net(regression=True, backbone=True)
    net.load_state_dict({**net.state_dict(), **params.init_params(5)})
    imgs = torch.rand(3, 3, 120, 160, generator=torch.Generator().manual_seed(4))
    P, n, _, _ = _keypoint_set([32, 27, 22], 15)
    seen = []
    image_features = net.image_features

    def spy(images, Ps, ns, *a, **kw):
        out = image_features(images, Ps, ns, *a, **kw)
        seen.append(out)
        return out

    net.image_features = spy
    try:
        index = net.enroll_images(imgs, P, n, device=DEV, sc_mode="f32", batch=2, layout="fp8+host")
    finally:
        net.image_features = image_features
    x = torch.cat([s[0][0].view(-1, 32, 768) for s in seen])
    w = torch.cat([s[1][0] for s in seen])
    same_fields8(index, net.enroll_keypoints(P, n, x, w, device=DEV, sc_mode="f32", batch=2, layout="fp8+host"))
    w8, ws = ops.rows_quant8(index.y.clone())
    assert torch.equal(_u8(index.y8.cpu()), _u8(w8)) and torch.equal(index.s8.cpu(), ws)


@pytest.mark.parametrize("coarse", ["fused", "any"])
def test_coarse_scores_are_the_dequantised_index(world, coarse):
    net, i8, hand = world["net"], world["index"]["fp8+host"], world["hand"]
    got = net.coarse_scores([world["probe"]] + world["pdicts"][:1], i8, coarse=coarse)
    want = net.coarse_scores([world["probe"]] + world["pdicts"][:1], hand, coarse=coarse)
    assert torch.equal(_bits(got), _bits(want)) and bool(torch.isfinite(got).all())
    sel = [3, 0, 2]
    assert torch.equal(_bits(net.coarse_scores(world["probe"], i8, select=sel, coarse=coarse)),
                       _bits(got[:1, torch.tensor(sel, device=DEV)]))
    many = net.coarse_scores_many(world["pset"], i8, coarse=coarse)
    assert torch.equal(_bits(many), _bits(net.coarse_scores_many(world["pset"], hand, coarse=coarse)))
    assert torch.equal(_bits(many), _bits(net.coarse_scores(world["pdicts"], i8, coarse=coarse)))


def test_shortlisted_identify_ranks_fp8_scores_and_runs_the_exact_stage(world):
    net, i8, f32 = world["net"], world["index"]["fp8+host"], world["index"]["f32"]
    M = 4
    res = net.identify(world["probe"], i8, topk=3, shortlist=M, chunks=2)
    assert torch.equal(_bits(res["coarse_all"]), _bits(net.coarse_scores(world["probe"], world["hand"])[0]))
    hi, hs = ops.rank_select(res["coarse_all"].cpu().view(1, -1), M)
    assert torch.equal(res["short_idx"].cpu(), hi[0]) and torch.equal(_bits(res["coarse_score"].cpu()), _bits(hs[0]))
    ref = net.identify(world["probe"], f32, topk=3, select=res["short_idx"], chunks=2)
    for k in OUT_KEYS:
        assert res[k].dtype == ref[k].dtype and torch.equal(res[k], ref[k]), k
    # the hand-built bf16 index scores the same bits, so the whole result is its result
    same_results(res, net.identify(world["probe"], world["hand"], topk=3, shortlist=M, chunks=2))


def test_identify_many_equals_the_per_probe_calls(world):
    """One box for the three probes and the whole gallery (shortlist = G): the grouped exact stage runs every
    pair in the box the one-probe call runs it in."""
    net, i8 = world["net"], world["index"]["fp8+host"]
    G = i8.G
    res = net.identify_many(world["pset"], i8, topk=3, shortlist=G)
    assert [r["group"][0] for r in res] == [0, 0, 0]
    for p, r in enumerate(res):
        ref = net.identify(world["pdicts"][p], i8, topk=3, shortlist=G)
        for k in OUT_KEYS + ("short_idx",):
            assert r[k].dtype == ref[k].dtype and torch.equal(r[k], ref[k]), (p, k)
        for k in ("coarse_score", "coarse_all"):
            assert torch.equal(_bits(r[k]), _bits(ref[k])), (p, k)
    same_results(net.identify_many(world["pset"], i8, topk=2, shortlist=3),
                 net.identify_many(world["pset"], world["hand"], topk=2, shortlist=3))


def test_subject_level_query(world):
    net, i8 = world["net"], world["index"]["fp8+host"]
    res = net.identify(world["probe"], i8, topk=2, shortlist=2, by="subject")
    same_results(res, net.identify(world["probe"], world["hand"], topk=2, shortlist=2, by="subject"))
    ref = net.identify(world["probe"], world["index"]["f32"], topk=2, select=res["short_idx"], by="subject")
    for k in ("cls_prob", "k_prob", "ds_mat", "perm_mat", "top_subject", "top_score"):
        assert torch.equal(res[k], ref[k]), k


def _queries8(net, probe, pset, index):
    return {"short": net.identify(probe, index, topk=3, shortlist=3),
            "short subject": net.identify([probe, probe], index, topk=2, shortlist=2, by="subject", threshold=0.5),
            "open": net.identify(probe, index, topk=2, shortlist=3, normalize="cohort", cohort=2, threshold=0.0),
            "coarse": net.coarse_scores(probe, index),
            "coarse many": net.coarse_scores_many(pset, index, coarse="any"),
            "many short": net.identify_many(pset, index, topk=3, shortlist=3),
            "many subject": net.identify_many(pset, index, topk=2, shortlist=2, by="subject")}


def test_mutable_index_equals_a_fresh_enrolment_of_the_survivors(world):
    net, kw = world["net"], world["kw"]
    whole = world["index"]["fp8+host"]
    GA = len(world["dA"])
    index = net.enroll(world["dA"], DEV, layout="fp8+host", subjects=world["sA"], capacity=whole.used, **kw)
    assert index.capacity == whole.used and index.y8.data_ptr() == index._store["y8"].data_ptr()
    new = net.enroll_into(index, world["dB"], batch=4, subjects=world["sB"])
    assert new.tolist() == list(range(GA, whole.G))
    same_fields8(index, whole, "enroll_into")
    kp = net.enroll_keypoints(*[t.to(DEV) for t in world["A"]], layout="fp8+host", subjects=world["sA"],
                              capacity=whole.used, **kw)
    net.enroll_keypoints_into(kp, *[t.to(DEV) for t in world["B"]], batch=4, subjects=world["sB"])
    same_fields8(kp, whole, "enroll_keypoints_into")
    gone = [1, GA]                                           # one of A, the first of B
    index.remove(gone)
    live = index.live.clone()
    ptr = index.y8.data_ptr()
    new_of_old = index.compact(stage_rows=int(whole.n.max()))
    assert index.last_compact["staged"] >= 1 and index.y8.data_ptr() == ptr and not index.tombstones
    assert new_of_old[live].tolist() == list(range(live.numel()))
    graphs, subj = world["dA"] + world["dB"], world["sA"] + world["sB"]
    fresh = net.enroll([graphs[e] for e in live.tolist()], DEV, layout="fp8+host",
                       subjects=[subj[e] for e in live.tolist()], **kw)
    same_fields8(index, fresh, "compact")
    same_fields8(index, whole.slice(live), "slice")
    got, want = _queries8(net, world["probe"], world["pset"], index), _queries8(net, world["probe"], world["pset"], fresh)
    for name in got:
        if isinstance(got[name], torch.Tensor):
            assert torch.equal(_bits(got[name]), _bits(want[name])), name
        else:
            same_results(got[name], want[name], name)
    far = whole.reserve(*whole.used)                         # one entry left at the end: storage to storage
    far.remove(list(range(whole.G - 1)))
    far.compact()
    assert far.last_compact == dict(direct=1, staged=0, launches=1, rows=int(whole.n[-1]))
    same_fields8(far, whole.slice(torch.tensor([whole.G - 1])))


def test_three_shards_on_one_gpu_equal_the_single_index(world):
    net, i8 = world["net"], world["index"]["fp8+host"]
    sg = ShardedGallery.split(i8, [0, 0, 0], torch.arange(i8.G) % 3)
    assert sg.layout == "fp8+host" and all(s.y8 is not None and s.y16 is None for s in sg.shards)
    for s, shard in enumerate(sg.shards):
        same_fields8(shard, i8.slice(torch.nonzero(torch.arange(i8.G) % 3 == s).view(-1)), s)
    probes = [world["probe"]] + world["pdicts"][:2]
    kw = dict(topk=3, shortlist=4)
    _check_against(net.identify(probes, sg, **kw), net.identify(probes, i8, **kw))
    whole = ShardedGallery.split(i8, [0, 0, 0], "subject")   # subjects whole inside a shard: the subject-level query
    kw = dict(topk=2, shortlist=2, by="subject")
    _check_against(net.identify(probes, whole, **kw), net.identify(probes, i8, **kw))

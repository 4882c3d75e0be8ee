"""Gallery over several GPUs on the device: ``fpm_topk_merge`` against its host statement, bit for bit, and
``Net.identify`` over a ``ShardedGallery`` (three shards on the one GPU) against the same query over the same
gallery in one index: every query key and every carried per-pair output, on bits."""
import ctypes

import pytest
import torch

from fpm import _lib, ops
from fpm.sharded_gallery import PAIR_KEYS, ShardedGallery
from test_shortlist_cpu import state_dicts
from test_shortlist_gpu import _net, planted
from test_sharded_gallery_cpu import merge_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = -7


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_merge(dev, host):
    """(top_id, top_score, top_col) of the device against the statement's, scores on bits."""
    for d, h, name in zip(dev, host, ("top_id", "top_score", "top_col")):
        assert d.dtype == h.dtype and tuple(d.shape) == tuple(h.shape), name
        assert torch.equal(_bits(d.cpu()), _bits(h)), name


def _device_merge(sc, ids, off, k):
    """``ops.topk_merge`` on the device over outputs prefilled with a sentinel: every slot must be written."""
    P = int(sc.shape[0])
    outs = (torch.full((P, k), SENTINEL, dtype=torch.int32, device=DEV), torch.full((P, k), float("nan"), device=DEV),
            torch.full((P, k), SENTINEL, dtype=torch.int32, device=DEV))
    got = ops.topk_merge(sc, ids, off, k, *outs)
    assert all(g is o for g, o in zip(got, outs))
    assert not bool((got[0] == SENTINEL).any()) and not bool((got[2] == SENTINEL).any())
    return got


# ---------------------------------------------------------------------------------------------- the kernel
LISTS = [([1], 1), ([7, 7, 7], 7), ([5, 0, 9], 6), ([64, 64, 41, 1], 64), ([1024] * 8, 1024), ([1024] * 16, 1024)]


@pytest.mark.parametrize("how", ["round-robin", "random"])
@pytest.mark.parametrize("P", [1, 3, 70])
@pytest.mark.parametrize("lengths,k", LISTS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_kernel_equals_statement(lengths, k, P, how):
    sc, ids, off = merge_case(lengths, P, how, 31 * len(lengths) + k)
    host = ops.topk_merge(sc, ids, off, k)
    dev = _device_merge(sc.to(DEV), ids.to(DEV), off, k)
    _same_merge(dev, host)
    # a row stride larger than L: views of wider tensors
    L = int(sc.shape[1])
    wide_s = torch.full((P, L + 9), float("nan"), device=DEV)
    wide_i = torch.full((P, L + 9), -1, dtype=torch.int32, device=DEV)
    wide_s[:, 4:4 + L], wide_i[:, 4:4 + L] = sc.to(DEV), ids.to(DEV)
    _same_merge(_device_merge(wide_s[:, 4:4 + L], wide_i[:, 4:4 + L], off, k), host)


def test_one_list_returns_its_first_k():
    sc, ids, off = merge_case([200], 3, "random", 5)
    ti, ts, tc = _device_merge(sc.to(DEV), ids.to(DEV), off, 77)
    assert torch.equal(ti.cpu(), ids[:, :77]) and torch.equal(_bits(ts.cpu()), _bits(sc[:, :77]))
    assert torch.equal(tc.cpu(), torch.arange(77, dtype=torch.int32).expand(3, 77))


def test_a_row_alone_equals_its_row_of_a_large_launch():
    sc, ids, off = merge_case([64, 64, 41, 1], 70, "round-robin", 8)
    full = _device_merge(sc.to(DEV), ids.to(DEV), off, 64)
    for p in (0, 33, 69):
        alone = _device_merge(sc[p:p + 1].to(DEV), ids[p:p + 1].to(DEV), off, 64)
        _same_merge(alone, [t[p:p + 1].cpu() for t in full])


def _c_call(lib, sc, ids, ld, P, off, S, k, outs):
    V = ctypes.c_void_p
    offs = (ctypes.c_int * len(off))(*off)
    ptr = lambda t: V(0 if t is None else t.data_ptr())
    return lib.fpm_topk_merge(ptr(sc), ptr(ids), ld, P, offs, S, k, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                              V(torch.cuda.current_stream(DEV).cuda_stream))


def test_c_abi_and_refusals_launch_nothing():
    lib = _lib.load()
    sc, ids, off = merge_case([5, 0, 9], 2, "random", 3)
    host = ops.topk_merge(sc, ids, off, 6)
    sd, idd = sc.to(DEV), ids.to(DEV)
    fresh = lambda: (torch.full((2, 6), SENTINEL, dtype=torch.int32, device=DEV),
                     torch.full((2, 6), float(SENTINEL), device=DEV),
                     torch.full((2, 6), SENTINEL, dtype=torch.int32, device=DEV))
    outs = fresh()
    assert _c_call(lib, sd, idd, 14, 2, off, 3, 6, outs) == 0
    _same_merge(outs, host)
    outs = fresh()
    before = [t.clone() for t in outs]
    bad = [
        (dict(S=0), b"lists"), (dict(S=17, off=list(range(18))), b"lists"),
        (dict(off=[1, 5, 5, 14]), b"start at 0"), (dict(off=[0, 6, 5, 14]), b"must not fall"),
        (dict(off=[0, 1025, 1025, 1030]), b"at most 1024"), (dict(off=[0, 0, 0, 0]), b"empty"),
        (dict(P=-1), b"rows"), (dict(P=65536), b"rows"), (dict(ld=13), b"stride"),
        (dict(k=0), b"topk_merge: k"), (dict(k=15), b"topk_merge: k"),
        (dict(off=[0, 1024, 2048, 3072], ld=3072, k=1025), b"topk_merge: k"),
        (dict(sc=None), b"required"), (dict(ids=None), b"required"), (dict(out=1), b"required"),
    ]
    for kw, msg in bad:
        o = list(outs)
        if "out" in kw:
            o[kw["out"]] = None
        a = dict(sc=sd, ids=idd, ld=14, P=2, off=off, S=3, k=6)
        a.update({k: v for k, v in kw.items() if k != "out"})
        rc = _c_call(lib, a["sc"], a["ids"], a["ld"], a["P"], a["off"], a["S"], a["k"], o)
        assert rc != 0 and msg in lib.fpm_last_error(), (kw, lib.fpm_last_error())
    V = ctypes.c_void_p
    rc = lib.fpm_topk_merge(V(sd.data_ptr()), V(idd.data_ptr()), 14, 2, None, 3, 6, V(outs[0].data_ptr()),
                            V(outs[1].data_ptr()), V(outs[2].data_ptr()), None)
    assert rc != 0 and b"list_off" in lib.fpm_last_error()
    # the wrapper's refusals on device tensors
    for kw, msg in ((dict(k=0), "topk_merge: k"), (dict(ids=idd.long()), "int32"), (dict(ids=ids), "is on"),
                    (dict(off=[0, 5, 5, 13]), "ends at")):
        a = dict(sc=sd, ids=idd, off=off, k=6)
        a.update(kw)
        with pytest.raises(_lib.FpmError, match=msg):
            ops.topk_merge(a["sc"], a["ids"], a["off"], a["k"])
    torch.cuda.synchronize()
    for t, b in zip(outs, before):
        assert torch.equal(_bits(t), _bits(b))


# ----------------------------------------------------------------------------------------------- the query
@pytest.fixture(scope="module")
def sds():
    return state_dicts()


@pytest.fixture(scope="module", params=["f32", "bf16"])
def world(request, sds):
    """The planted gallery (40 entries of 24-48 keypoints, three probes, labels e // 3) enrolled in one index per
    layout, with a cache of the one-index reference queries."""
    gal, probes = planted()
    net = _net(sds["spread"], request.param)
    labels = [e // 3 for e in range(len(gal))]
    index = {layout: net.enroll(gal, DEV, batch=16, layout=layout, subjects=labels) for layout in ("f32", "bf16+host")}
    return dict(net=net, probes=probes, index=index, labels=labels, G=len(gal), refs={}, split={})


def _reference(world, layout, **kw):
    key = (layout,) + tuple(sorted(kw.items()))
    if key not in world["refs"]:
        world["refs"][key] = world["net"].identify(world["probes"], world["index"][layout], **kw)
    return world["refs"][key]


def _assign(world, how):
    G = world["G"]
    return torch.arange(G) % 3 if how == "round-robin" else how


def _split(world, layout, how):
    key = (layout, how)
    if key not in world["split"]:
        world["split"][key] = ShardedGallery.split(world["index"][layout], [0, 0, 0], _assign(world, how))
    return world["split"][key]


def _check_against(res, ref, coarse_all=True):
    """Every key of the sharded results is the reference's, on bits; the keys left out are the forward's
    batch-level ones."""
    assert len(res) == len(ref)
    for p, (r, b) in enumerate(zip(res, ref)):
        carried = {k for k, v in b.items() if k in PAIR_KEYS}
        query = set(b) - {"cls_loss", "ks_loss", "ks_error", "lsa", "sk_steps", "Kp", "coef", "ss64"} - set(PAIR_KEYS)
        want = carried | query if coarse_all else (carried | query) - {"coarse_all"}
        assert set(r) == want, (p, sorted(set(r) ^ want))
        assert {"s", "ss", "ds_mat", "perm_mat", "k_prob", "cls_prob", "cls_logits"} <= carried
        for key in sorted(want):
            a, v = r[key], b[key]
            assert a.dtype == v.dtype and tuple(a.shape) == tuple(v.shape) and a.device == v.device, (p, key)
            same = torch.equal(_bits(a), _bits(v)) if v.dtype == torch.float32 else torch.equal(a, v)
            assert same, (p, key)


@pytest.mark.parametrize("score", ["cls_prob", "k_prob"])
@pytest.mark.parametrize("M", [8, 40])
@pytest.mark.parametrize("layout", ["f32", "bf16+host"])
@pytest.mark.parametrize("how", ["range", "round-robin"])
def test_entry_level_query_equals_one_index(world, how, layout, M, score):
    kw = dict(topk=5, shortlist=M, score=score)
    ref = _reference(world, layout, **kw)
    sg = _split(world, layout, how)
    # the test's own inputs, from the reference alone: a shortlist that draws on several shards, and a shard
    # whose part of a list is smaller than the list's box (pad_to at work)
    several = smaller = False
    for b in ref:
        ent = b["short_idx"].cpu().long()
        own = sg.owner[ent]
        several |= int(torch.unique(own).numel()) >= 2
        smaller |= any(int(sg.n[ent[own == s]].max()) < int(sg.n[ent].max()) for s in torch.unique(own).tolist())
    assert several and smaller, (several, smaller)
    res = world["net"].identify(world["probes"], sg, **kw)
    _check_against(res, ref)
    assert all(r["short_idx"].numel() == min(M, world["G"]) for r in res)


def test_one_probe_and_coarse_all_off(world):
    sg = _split(world, "f32", "range")
    ref = _reference(world, "f32", topk=5, shortlist=8, score="cls_prob")
    one = world["net"].identify(world["probes"][1], sg, topk=5, shortlist=8)
    assert isinstance(one, dict)
    _check_against([one], [ref[1]])
    res = world["net"].identify(world["probes"], sg, topk=5, shortlist=8, coarse_all=False)
    _check_against(res, ref, coarse_all=False)
    assert world["net"].identify([], sg, shortlist=8) == []


@pytest.mark.parametrize("kw", [
    dict(fuse="max", impressions="all"), dict(fuse="mean", impressions="all"), dict(fuse="max", impressions="best"),
    dict(fuse="mean", impressions="best"), dict(fuse="mean", top_r=2),
    dict(fuse="mean", normalize="cohort", cohort=4, threshold=0.5),
    dict(fuse="mean", top_r=2, normalize="cohort", cohort=4, threshold=0.5, shortlist=40),
], ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_subject_level_query_equals_one_index(world, kw):
    kw = dict(dict(topk=5, shortlist=8, by="subject"), **kw)
    sg = _split(world, "f32", "subject")
    assert not sg.subject_split
    ref = _reference(world, "f32", **kw)
    assert any(int(torch.unique(sg.owner[b["short_idx"].cpu().long()]).numel()) >= 2 for b in ref)
    _check_against(world["net"].identify(world["probes"], sg, **kw), ref)


def test_entry_level_open_set_equals_one_index(world):
    kw = dict(topk=5, shortlist=8, normalize="cohort", cohort=4, threshold=0.5)
    _check_against(world["net"].identify(world["probes"], _split(world, "f32", "round-robin"), **kw),
                   _reference(world, "f32", **kw))


def test_constructor_over_sliced_parts_equals_split(world):
    index = world["index"]["f32"]
    deal = torch.arange(world["G"]) % 3
    entry = [torch.nonzero(deal == s).view(-1) for s in range(3)]
    sg = ShardedGallery([index.slice(e, DEV) for e in entry], entry, output_device=0)
    cut = _split(world, "f32", "round-robin")
    assert sg.owner.tolist() == cut.owner.tolist() and sg.local.tolist() == cut.local.tolist()
    assert sg.devices == [DEV] * 3 and sg.output_device == DEV
    for a, b in zip(sg.shards, cut.shards):
        for name in ("y", "row_off", "n", "src", "dst", "pseudo", "edge_off", "w", "P", "subject"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
    kw = dict(topk=5, shortlist=8, score="cls_prob")
    _check_against(world["net"].identify(world["probes"], sg, **kw), _reference(world, "f32", **kw))


def test_query_refusals(world):
    net, probes = world["net"], world["probes"]
    sg = _split(world, "f32", "range")
    with pytest.raises(_lib.FpmError, match="shortlist=None"):
        net.identify(probes, sg)
    with pytest.raises(_lib.FpmError, match="select"):
        net.identify(probes, sg, shortlist=8, select=[0, 1])
    # labels e // 3 and contiguous ranges of 14, 13, 13 entries: subject 4 is cut
    assert sg.subject_split
    with pytest.raises(_lib.FpmError, match="by='subject'"):
        net.identify(probes, sg, shortlist=8, by="subject")
    assert len(net.identify(probes, sg, shortlist=8)) == 3                 # fine at entry level
    pset = net.enroll(probes, DEV, batch=2)
    for call in (lambda: net.identify_many(pset, sg, shortlist=8), lambda: net.coarse_scores_many(pset, sg),
                 lambda: net.match_pairs(pset, sg, [[0, 0]])):
        with pytest.raises(_lib.FpmError, match="ShardedGallery"):
            call()
    for bad, msg in ((dict(shortlist=0), "shortlist"), (dict(shortlist=8, score="x"), "score"),
                     (dict(shortlist=8, coarse="x"), "coarse"), (dict(shortlist=8, impressions="best"), "impressions"),
                     (dict(shortlist=8, top_r=2), "top_r")):
        with pytest.raises(_lib.FpmError, match=msg):
            net.identify(probes, sg, **bad)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two or more GPUs (distinct devices)")
@pytest.mark.parametrize("M", [8, 40])
def test_distinct_devices_equal_one_index(world, M):
    devices = list(range(min(3, torch.cuda.device_count())))
    sg = ShardedGallery.split(world["index"]["f32"], devices, "range")
    kw = dict(topk=5, shortlist=M, score="cls_prob")
    _check_against(world["net"].identify(world["probes"], sg, **kw), _reference(world, "f32", **kw))

"""Mutable gallery index on the GPU: the ragged segment-copy kernel against its torch statement (bit for bit,
storage to storage and through a stage), ``Net.enroll_into`` / ``enroll_keypoints_into`` against the separate
enrolment of the appended graphs (every field), a failed append, queries over an index with removed entries
against the untouched twin with ``select=live``, ``compact`` against ``slice(live)``, and a ShardedGallery over a
shard that changed."""
import pytest
import torch

from fpm import _lib, ops, params
from fpm.sharded_gallery import ShardedGallery
from test_enroll_keypoints_gpu import CASES, DEV, LAYOUTS, OUT_KEYS, _export, _keypoint_set, _net
from test_mutable_index_cpu import _bits, move_case, move_statement, moved_specials, same_fields

pytestmark = pytest.mark.gpu

APPENDED = {"f32ops-f32": [44, 48, 31], "f32ops-bf16": [44, 48, 31], "bf16ops": [72, 33]}
SUBJECTS = {6: [0, 0, 1, 2, 1, 3], 4: [0, 0, 1, 1], 3: [2, 4, 4], 2: [1, 2]}
QUERY_KEYS = ("top_idx", "top_score", "short_idx", "short_off", "coarse_score", "coarse_all", "subjects",
              "subject_score", "top_subject", "short_subject", "coarse_subject_score", "top_z", "cohort_mu",
              "cohort_sigma", "cohort_n", "accept", "match")
ALL_KEYS = OUT_KEYS + ("cls_logits",) + QUERY_KEYS


def _same_bits(a, b, what):
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for u, v in zip(a, b):
            _same_bits(u, v, what)
        return
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), what
    assert torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8)), what


def same_results(got, want, what="", entry_map=None):
    """Every key of ALL_KEYS that a result carries, bit for bit; ``entry_map`` (device int64): the entry
    numbers of ``want`` renumbered before the comparison (a compacted index against its twin)."""
    if isinstance(got, list):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            same_results(g, w, (what, i), entry_map)
        return
    assert {k for k in ALL_KEYS if k in got} == {k for k in ALL_KEYS if k in want}, what
    for k in ALL_KEYS:
        if k not in got:
            continue
        w = want[k]
        if entry_map is not None and (k in ("top_idx", "short_idx") or (k == "match" and "top_subject" not in want)):
            ren = lambda t: torch.where(t >= 0, entry_map[t.long().clamp(min=0)], t.long()).to(t.dtype)
            w = [ren(t) for t in w] if isinstance(w, (list, tuple)) else ren(w)
        _same_bits(got[k], w, (what, k))


# --------------------------------------------------------------------------------------- rows_move
@pytest.mark.parametrize("which", ["f32", "b16", "both"])
def test_rows_move_bits(which):
    """The host case on the device, bit for bit against the statement: to another buffer (NaN fill kept outside
    the ranges), inside one buffer with disjoint ranges, and through a stage where a destination meets a source."""
    src, so, do, cnt, rows = move_case()
    s16 = src.to(torch.bfloat16)
    s16.view(torch.int16)[int(so[3]), 7] = 0x7FC1
    for rows_ in (src, s16):                                   # NaN, +-inf, -0 and subnormals are in the rows that move
        moved_specials(rows_, so, cnt)
    f32, b16 = which != "b16", which != "f32"
    dev = lambda t: None if t is None else t.to(DEV)
    s32_d, s16_d = dev(src) if f32 else None, dev(s16) if b16 else None
    d32 = torch.full((rows + 3, 768), float("nan"), device=DEV) if f32 else None
    d16 = torch.full((rows + 3, 768), float("nan"), device=DEV, dtype=torch.bfloat16) if b16 else None
    ops.rows_move(so.to(DEV), do.to(DEV), cnt.to(DEV), src32=s32_d, dst32=d32, src16=s16_d, dst16=d16,
                  src_off_host=so, dst_off_host=do, cnt_host=cnt)
    torch.cuda.synchronize()
    for got, s in ((d32, src), (d16, s16)):
        if got is not None:
            want = move_statement(s, so, do, cnt, torch.full((rows + 3, 768), float("nan"), dtype=s.dtype))
            assert torch.equal(_bits(got.cpu()), _bits(want))
    # inside one buffer: the segments moved to the front of their own storage, through a stage and directly
    so2 = torch.tensor([3, 30, 50, 90], dtype=torch.int64)
    cn2 = torch.tensor([17, 16, 33, 1], dtype=torch.int64)
    do2 = torch.cat([torch.zeros(1, dtype=torch.int64), cn2.cumsum(0)[:-1]])
    st2 = do2.clone()
    for rows_ in (src, s16):
        moved_specials(rows_, so2, cn2)
    with pytest.raises(_lib.FpmError, match="a destination range meets a source range"):
        ops.rows_move(so2.to(DEV), do2.to(DEV), cn2.to(DEV), src32=s32_d, dst32=s32_d, src16=s16_d, dst16=s16_d)
    g32 = torch.empty(67, 768, device=DEV) if f32 else None
    g16 = torch.empty(67, 768, device=DEV, dtype=torch.bfloat16) if b16 else None
    ops.rows_move(so2.to(DEV), st2.to(DEV), cn2.to(DEV), src32=s32_d, dst32=g32, src16=s16_d, dst16=g16)
    ops.rows_move(st2.to(DEV), do2.to(DEV), cn2.to(DEV), src32=g32, dst32=s32_d, src16=g16, dst16=s16_d)
    far, near, cn3 = torch.tensor([80, 90]), torch.tensor([67, 74]), torch.tensor([7, 6])    # 80 .. 96 to 67 .. 80
    ops.rows_move(far.to(DEV), near.to(DEV), cn3.to(DEV), src32=s32_d, dst32=s32_d, src16=s16_d, dst16=s16_d)
    torch.cuda.synchronize()
    for got, s in ((s32_d, src), (s16_d, s16)):
        if got is not None:
            want = move_statement(s.clone(), so2, do2, cn2, s.clone())
            want = move_statement(want.clone(), far, near, cn3, want)
            assert torch.equal(_bits(got.cpu()), _bits(want))


# -------------------------------------------------------------------------------------- the galleries
@pytest.fixture(scope="module")
def sd():
    return params.init_params(7)


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request, sd):
    dtype, n_probe, ns, sc_mode = CASES[request.param]
    net = _net(sd, dtype)
    A, B = _keypoint_set(ns, 11), _keypoint_set(APPENDED[request.param], 21)
    dA, dB = _export(*A), _export(*B)
    probe = _export(*_keypoint_set([n_probe], 12))[0]
    nmax = max(ns)
    pset = net.enroll_keypoints(*_keypoint_set([nmax - 8, nmax, nmax - 15], 13), device=DEV, sc_mode=sc_mode, batch=2)
    return dict(net=net, A=A, B=B, dA=dA, dB=dB, probe=probe, pset=pset, sc_mode=sc_mode,
                sA=SUBJECTS[len(dA)], sB=SUBJECTS[len(dB)], cache={})


def _enrolled(case, which, layout):
    """``Net.enroll`` of A, B or A + B alone (batch 4, labelled), made once per layout and left unchanged."""
    key = (which, layout)
    if key not in case["cache"]:
        graphs = {"A": case["dA"], "B": case["dB"], "AB": case["dA"] + case["dB"]}[which]
        subj = {"A": case["sA"], "B": case["sB"], "AB": case["sA"] + case["sB"]}[which]
        case["cache"][key] = case["net"].enroll(graphs, DEV, sc_mode=case["sc_mode"], batch=4, layout=layout,
                                                subjects=subj)
    return case["cache"][key]


def _capacity(case, spare=0):
    a, b = _enrolled(case, "A", "f32"), _enrolled(case, "B", "f32")
    return tuple(u + v + spare for u, v in zip(a.used, b.used))


def _mutable(case, layout, spare=0):
    """A fresh index of A with room for B (and ``spare``), by ``reserve``."""
    return _enrolled(case, "A", layout).reserve(*_capacity(case, spare))


def check_followed_by(index, first, second):
    """Every field of ``index`` is ``first``'s followed by ``second``'s, offsets shifted."""
    G, R, E = first.used
    assert index.used == tuple(u + v for u, v in zip(first.used, second.used))
    same_fields(index.slice(torch.arange(G)), first, "first")
    same_fields(index.slice(torch.arange(G, index.G)), second, "second")
    assert torch.equal(index.row_off_host[G:] - R, second.row_off_host)
    assert torch.equal(index.edge_off[G:] - E, second.edge_off)
    assert torch.equal(index.row_off.cpu(), index.row_off_host) and index.y.is_cuda == (index.layout != "bf16+host")
    for k in ("y", "y16", "P", "src", "dst", "pseudo", "w"):
        if getattr(index, k) is not None:
            assert torch.equal(_bits(getattr(index, k).cpu()),
                               _bits(torch.cat([getattr(first, k), getattr(second, k)]).cpu())), k


@pytest.mark.parametrize("route", ["dicts", "keypoints"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_enroll_into_equals_separate_enrolment(case, layout, route):
    net, kw = case["net"], dict(sc_mode=case["sc_mode"], batch=4, layout=layout, subjects=case["sA"])
    cap = _capacity(case)
    if route == "dicts":
        index = net.enroll(case["dA"], DEV, capacity=cap, **kw)
    else:
        index = net.enroll_keypoints(*[t.to(DEV) for t in case["A"]], capacity=cap, **kw)
    first, second = _enrolled(case, "A", layout), _enrolled(case, "B", layout)
    same_fields(index, first, "enrolled with capacity")
    assert index.capacity == cap and index.generation == 0 and index.used == first.used
    ptr = index.y.data_ptr()
    if route == "dicts":
        new = net.enroll_into(index, case["dB"], batch=4, subjects=case["sB"])
    else:
        new = net.enroll_keypoints_into(index, *[t.to(DEV) for t in case["B"]], batch=4, subjects=case["sB"])
    assert new.tolist() == list(range(first.G, first.G + second.G)) and index.generation == 1
    assert index.y.data_ptr() == ptr and index.used == index.capacity
    check_followed_by(index, first, second)
    whole = _enrolled(case, "AB", layout)
    for kws in (dict(shortlist=4), {}):
        got = net.identify(case["probe"], index, topk=3, chunks=2, **kws)
        want = net.identify(case["probe"], whole, topk=3, chunks=2, **kws)
        for k in OUT_KEYS + ("top_idx", "top_score") + (("short_idx",) if kws else ()):
            assert torch.equal(got[k], want[k]), (k, kws)


@pytest.mark.parametrize("route", ["dicts", "keypoints"])
def test_failed_append_leaves_index_unchanged(case, route):
    """B is cut into two sub-batches; the edge capacity ends one edge short of the second."""
    net, layout = case["net"], "bf16+host"
    batch = len(case["dB"]) - 1
    first, second = _enrolled(case, "A", layout), _enrolled(case, "B", layout)
    cap = _capacity(case)
    index = first.reserve(cap[0], cap[1], cap[2] - 1)
    assert 0 < int(second.edge_off[batch]) < int(second.edge_off[-1])           # the first sub-batch fits
    before = net.identify(case["probe"], index, topk=3, chunks=2, shortlist=4)
    gen, used, ptr = index.generation, index.used, index.y.data_ptr()
    with pytest.raises(_lib.FpmError, match="edges pass the index's capacity"):
        if route == "dicts":
            net.enroll_into(index, case["dB"], batch=batch, subjects=case["sB"])
        else:
            net.enroll_keypoints_into(index, *[t.to(DEV) for t in case["B"]], batch=batch, subjects=case["sB"])
    assert (index.generation, index.used, index.y.data_ptr()) == (gen, used, ptr)
    same_fields(index, first)
    same_results(net.identify(case["probe"], index, topk=3, chunks=2, shortlist=4), before)
    # refused before any launch
    for bad, why in ((dict(subjects=None), "has subject labels"), (dict(subjects=case["sB"] + [1]), "subject labels")):
        with pytest.raises(_lib.FpmError, match=why):
            net.enroll_into(index, case["dB"], **bad)
    with pytest.raises(_lib.FpmError, match="has no capacity"):
        net.enroll_into(first, case["dB"], subjects=case["sB"])
    with pytest.raises(_lib.FpmError, match="pass the index's capacity"):
        net.enroll_into(index, case["dB"] + case["dB"], subjects=case["sB"] + case["sB"])
    other = _net(params.init_params(8), net.dtype_mode)
    with pytest.raises(_lib.FpmError, match="other SplineConv weights"):
        other.enroll_into(index, case["dB"], subjects=case["sB"])
    same_fields(index, first)
    assert index.generation == gen


def _queries(net, probe, pset, index, live=None, plive=None, few=False):
    """Every query form over ``index`` (``live``: the twin's ``select``; ``plive``: its ``probe_select`` where
    the index is its own probe set; ``few``: one form of each call) -> {name: result}."""
    sel = {} if live is None else dict(select=live)
    own = {} if live is None else dict(select=live, probe_select=plive)
    out = {}
    if few:
        out["short"] = net.identify(probe, index, topk=3, shortlist=3, by="subject", **sel)
        out["many short"] = net.identify_many(pset, index, topk=3, shortlist=3, **sel)
        return out
    if index.layout != "bf16+host":
        out["identify"] = net.identify(probe, index, topk=3, chunks=2, **sel)
        out["identify subject"] = net.identify(probe, index, topk=3, by="subject", fuse="mean", **sel)
        out["many"] = net.identify_many(pset, index, topk=3, **sel)
        out["self"] = net.identify_many(index, index, topk=3, shortlist=3, exclude_self=True, **own)
        out["self subject"] = net.identify_many(index, index, topk=2, shortlist=2, exclude_self=True, by="subject", **own)
        out["as probes"] = net.identify_many(index, pset, topk=2, shortlist=2,
                                             **({} if plive is None else dict(probe_select=plive)))
        out["pairs many"] = net.coarse_scores_many(index, pset, **({} if plive is None else dict(probe_select=plive)))
    out["short"] = net.identify(probe, index, topk=3, shortlist=3, **sel)
    out["short subject"] = net.identify([probe, probe], index, topk=2, shortlist=2, by="subject", threshold=0.5, **sel)
    out["open"] = net.identify(probe, index, topk=2, shortlist=3, normalize="cohort", cohort=2, threshold=0.0, **sel)
    out["coarse"] = net.coarse_scores(probe, index, **sel)
    out["coarse many"] = net.coarse_scores_many(pset, index, **sel)
    out["many short"] = net.identify_many(pset, index, topk=3, shortlist=3, **sel)
    out["many subject"] = net.identify_many(pset, index, topk=2, shortlist=2, by="subject", threshold=0.5, **sel)
    return out


def _compare(got, want, entry_map=None):
    """``entry_map`` renumbers the entries of ``want`` -- but not where the index is the probe set: the entries
    those results name are the other index's."""
    assert sorted(got) == sorted(want)
    for name in got:
        if isinstance(got[name], torch.Tensor):
            _same_bits(got[name], want[name], name)
        else:
            same_results(got[name], want[name], name, None if name == "as probes" else entry_map)


def _gone(index):
    return [1, 4] if index.G == 6 else [1]


@pytest.mark.parametrize("layout", ["f32+bf16", "bf16+host"])
def test_removed_entries_equal_select(case, layout):
    net, twin = case["net"], _enrolled(case, "A", layout)
    index = twin.reserve(*twin.used)
    index.remove(_gone(index))
    live = index.live
    assert live.numel() == twin.G - len(_gone(index)) and index.G == twin.G
    _compare(_queries(net, case["probe"], case["pset"], index),
             _queries(net, case["probe"], case["pset"], twin, live, live))
    for call in (lambda s: net.identify(case["probe"], index, select=s, shortlist=2),
                 lambda s: net.coarse_scores(case["probe"], index, select=s),
                 lambda s: net.identify_many(case["pset"], index, select=s, shortlist=2),
                 lambda s: net.coarse_scores_many(case["pset"], index, select=s),
                 lambda s: net.match_pairs(case["pset"], index, [[0, s[0]]])):
        with pytest.raises(_lib.FpmError, match="entry 1 was removed"):
            call([1, 0])
    if layout != "bf16+host":
        with pytest.raises(_lib.FpmError, match="entry 1 was removed"):
            net.identify_many(index, case["pset"], probe_select=[1], shortlist=2)
        with pytest.raises(_lib.FpmError, match="entry 1 was removed"):
            net.match_pairs(index, case["pset"], [[1, 0]])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_compact_equals_slice(case, layout):
    net, twin, second = case["net"], _enrolled(case, "A", layout), _enrolled(case, "B", layout)
    index = _mutable(case, layout)
    index.remove(_gone(index))
    live = index.live.clone()
    ptr, cap = index.y.data_ptr(), index.capacity
    new_of_old = index.compact(stage_rows=int(twin.n.max()))
    want = twin.slice(live)
    same_fields(index, want)
    assert index.y.data_ptr() == ptr and index.capacity == cap and not index.tombstones
    assert new_of_old[live].tolist() == list(range(live.numel())) and int((new_of_old < 0).sum()) == len(_gone(twin))
    routes = index.last_compact
    assert routes["staged"] >= 1 and routes["launches"] == routes["direct"] + 2 * routes["staged"]
    got = _queries(net, case["probe"], case["pset"], index)
    ref = _queries(net, case["probe"], case["pset"], twin, live, live)
    _compare(got, ref, new_of_old.to(DEV))
    # the compacted index goes on: an append into the freed room, and the queries again
    new = net.enroll_into(index, case["dB"], batch=4, subjects=case["sB"])
    assert new.tolist() == list(range(live.numel(), live.numel() + second.G))
    check_followed_by(index, want, second)
    fresh = want.reserve(*cap)
    net.enroll_keypoints_into(fresh, *[t.to(DEV) for t in case["B"]], batch=4, subjects=case["sB"])
    _compare(_queries(net, case["probe"], case["pset"], index, few=True),
             _queries(net, case["probe"], case["pset"], fresh, few=True))
    # the far route: one entry left at the end lands before its own start, storage to storage
    far = twin.reserve(*twin.used)
    far.remove(list(range(twin.G - 1)))
    far.compact()
    assert far.last_compact == dict(direct=1, staged=0, launches=1, rows=int(twin.n[-1]))
    same_fields(far, twin.slice(torch.tensor([twin.G - 1])))


def test_sharded_refuses_changed_shard(case):
    net = case["net"]
    sg = ShardedGallery.split(_enrolled(case, "A", "f32"), [0, 0])
    net.identify(case["probe"], sg, shortlist=2, topk=2)
    sg.shards[1].remove([0])
    with pytest.raises(_lib.FpmError, match="shard 1 has changed since this ShardedGallery was built"):
        net.identify(case["probe"], sg, shortlist=2, topk=2)
    with pytest.raises(_lib.FpmError, match="a shard has removed entries"):
        ShardedGallery(sg.shards)
    sg.shards[1].compact()
    again = ShardedGallery(sg.shards)
    assert again.G == sg.G - 1
    net.identify(case["probe"], again, shortlist=2, topk=2)


def test_enroll_images_into_on_captured_features():
    """The image route: two images enrolled with capacity, a third enrolled into the index; the features are
    captured by a spy on ``net.image_features`` (MIOpen's are not reproducible call to call), and the index
    equals ``enroll_keypoints`` of the three on those features with the same sub-batches."""
    import fpm
    net = fpm.Net(regression=True, backbone=True)
    net.load_state_dict({**net.state_dict(), **params.init_params(5)})
    g = torch.Generator().manual_seed(4)
    imgs = torch.rand(3, 3, 120, 160, generator=g)
    P, n, _, _ = _keypoint_set([32, 27, 22], 15)
    seen = []
    image_features = net.image_features

    def spy(images, Ps, ns, *a, **kw):
        out = image_features(images, Ps, ns, *a, **kw)
        seen.append(out)
        return out

    net.image_features = spy
    try:
        index = net.enroll_images(imgs[:2], P[:2], n[:2], device=DEV, sc_mode="f32", batch=2, layout="f32+bf16",
                                  capacity=(4, 100))
        new = net.enroll_images_into(index, imgs[2:], P[2:], n[2:], batch=2)
    finally:
        net.image_features = image_features
    assert new.tolist() == [2] and index.used[:2] == (3, 81) and index.capacity == (4, 100, 600) and len(seen) == 2
    x = torch.cat([s[0][0].view(-1, 32, 768) for s in seen])
    w = torch.cat([s[1][0] for s in seen])
    # the pack generation counts packs, not weights: the net packed again between the two enrolments
    same_fields(index, net.enroll_keypoints(P, n, x, w, device=DEV, sc_mode="f32", batch=2, layout="f32+bf16"),
                pack_gen=False)

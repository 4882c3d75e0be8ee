"""Gallery over several GPUs, the parts that need none: ``ops.topk_merge``'s host statement against a numpy
sort of its key, the merge property (per-shard ``rank_select``, the id map and ``topk_merge`` equal
``rank_select`` of the whole row), the refusals, ``GalleryIndex.slice`` on a CPU-device index and the tables
of ``ShardedGallery``."""
import numpy as np
import pytest
import torch

import fpm
from fpm import _lib, ops
from fpm.gallery import GalleryIndex
from fpm.sharded_gallery import ShardedGallery
from test_shortlist_cpu import rank_scores

# (P, G, M, shards): the cases of the merge property
PROPERTY_CASES = [(3, 300, 7, 3), (2, 1000, 64, 4), (2, 3000, 1024, 8), (2, 41, 40, 3), (1, 50, 16, 16)]
ASSIGNS = ("round-robin", "contiguous", "random")


def _bits(t):
    return t.contiguous().view(torch.int32)


def assignment(G, S, how, seed=0):
    """The shard number of each of G entries."""
    if how == "round-robin":
        return torch.arange(G) % S
    if how == "contiguous":
        return (torch.arange(G) * S) // G
    return torch.randint(0, S, (G,), generator=torch.Generator().manual_seed(seed))


def shard_lists(s, shard, S, M):
    """Per shard ``rank_select`` to min(M, G_s) and the map to global numbers -> (score (P, L), ids (P, L)
    int32, list_off): what ``topk_merge`` takes.  A shard without entries gives an empty list."""
    sc, ids, off = [], [], [0]
    for t in range(S):
        e = torch.nonzero(shard == t).view(-1)
        k = min(M, int(e.numel()))
        if k:
            pi, ps = ops.rank_select(s[:, e].contiguous(), k)
            sc.append(ps)
            ids.append(e[pi.long()].to(torch.int32))
        off.append(off[-1] + k)
    return torch.cat(sc, 1), torch.cat(ids, 1), off


def merge_case(lengths, P, how, seed):
    """Lists of the given lengths cut from ``rank_scores`` rows over a gallery three times their total, the
    entries dealt to the shards by ``how``: ties are decided across lists."""
    S, total = len(lengths), sum(lengths)
    G = 3 * total + S
    s = rank_scores(P, G, seed)
    shard = assignment(G, S, how, seed)
    sc, ids, off = [], [], [0]
    for t, k in enumerate(lengths):
        e = torch.nonzero(shard == t).view(-1)
        assert e.numel() >= k
        if k:
            pi, ps = ops.rank_select(s[:, e].contiguous(), k)
            sc.append(ps)
            ids.append(e[pi.long()].to(torch.int32))
        off.append(off[-1] + k)
    return torch.cat(sc, 1), torch.cat(ids, 1), off


def _key_numpy(s, ids):
    s = np.asarray(s, dtype=np.float32)
    u = s.view(np.uint32).astype(np.uint64)
    bits = np.where(u >> np.uint64(31) != 0, np.uint64(0xFFFFFFFF) - u, u | np.uint64(0x80000000))
    bits = np.where(np.isnan(s), np.uint64(0), bits)
    return (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(ids).astype(np.uint64))


@pytest.mark.parametrize("lengths,k,P", [([1], 1, 1), ([7, 7, 7], 7, 3), ([5, 0, 9], 6, 2), ([64, 64, 41, 1], 64, 3),
                                         ([300] * 5, 1024, 2)])
@pytest.mark.parametrize("how", ["round-robin", "random"])
def test_host_statement_against_numpy(lengths, k, P, how):
    sc, ids, off = merge_case(lengths, P, how, 11 + k)
    ti, ts, tc = ops.topk_merge(sc, ids, off, k)
    key = _key_numpy(sc.numpy(), ids.numpy())
    order = np.argsort(np.uint64(0xFFFFFFFFFFFFFFFF) - key, axis=1, kind="stable")[:, :k]
    assert ti.dtype == torch.int32 and tc.dtype == torch.int32 and ts.dtype == torch.float32
    assert tuple(ti.shape) == tuple(ts.shape) == tuple(tc.shape) == (P, k)
    assert np.array_equal(tc.numpy(), order.astype(np.int32))
    assert np.array_equal(ti.numpy(), np.take_along_axis(ids.numpy(), order, 1))
    assert np.array_equal(ts.numpy().view(np.uint32), np.take_along_axis(sc.numpy(), order, 1).view(np.uint32))


@pytest.mark.parametrize("how", ASSIGNS)
@pytest.mark.parametrize("P,G,M,S", PROPERTY_CASES)
def test_merge_of_shard_shortlists_is_the_global_shortlist(P, G, M, S, how):
    s = rank_scores(P, G, G)
    sc, ids, off = shard_lists(s, assignment(G, S, how), S, M)
    k = min(M, G)
    ti, ts, tc = ops.topk_merge(sc, ids, off, k)
    ri, rs = ops.rank_select(s, k)
    assert torch.equal(ti, ri) and torch.equal(_bits(ts), _bits(rs))
    assert torch.equal(torch.gather(ids, 1, tc.long()), ti)


def test_topk_merge_refusals():
    sc, ids, off = merge_case([5, 0, 9], 2, "random", 3)
    ok = lambda **kw: ops.topk_merge(kw.get("sc", sc), kw.get("ids", ids), kw.get("off", off), kw.get("k", 6))
    ok()
    for k in (0, 15, -1):
        with pytest.raises(_lib.FpmError, match="topk_merge: k"):
            ok(k=k)
    with pytest.raises(_lib.FpmError, match="fp32"):
        ok(sc=sc.double())
    with pytest.raises(_lib.FpmError, match="int32"):
        ok(ids=ids.long())
    with pytest.raises(_lib.FpmError, match="shape"):
        ok(ids=ids[:, :-1])
    with pytest.raises(_lib.FpmError, match="start at 0"):
        ok(off=[1, 5, 5, 14])
    with pytest.raises(_lib.FpmError, match="must not fall"):
        ok(off=[0, 6, 5, 14])
    with pytest.raises(_lib.FpmError, match="ends at"):
        ok(off=[0, 5, 5, 13])
    with pytest.raises(_lib.FpmError, match="S \\+ 1"):
        ok(off=[0])
    with pytest.raises(_lib.FpmError, match="17 lists"):
        ops.topk_merge(torch.zeros(1, 17), torch.arange(17, dtype=torch.int32).view(1, 17), list(range(18)), 1)
    with pytest.raises(_lib.FpmError, match="at most 1024"):
        ops.topk_merge(torch.zeros(1, 1025), torch.arange(1025, dtype=torch.int32).view(1, 1025), [0, 1025], 1)
    with pytest.raises(_lib.FpmError, match="65535"):
        ops.topk_merge(torch.zeros(65536, 1), torch.zeros(65536, 1, dtype=torch.int32), [0, 1], 1)
    # the precondition, checked on the CPU path: a list out of order, an id twice, a negative id
    bad = sc.clone()
    bad[1, 7], bad[1, 8] = sc[1, 8], sc[1, 7]
    swapped = ids.clone()
    swapped[1, 7], swapped[1, 8] = ids[1, 8], ids[1, 7]
    assert not torch.equal(_bits(bad), _bits(sc)) or not torch.equal(swapped, ids)
    with pytest.raises(_lib.FpmError, match="strictly descending"):
        ok(sc=bad, ids=swapped)
    twice = ids.clone()
    twice[0, 2] = ids[0, 9]
    with pytest.raises(_lib.FpmError, match="twice|strictly descending"):
        ok(ids=twice)
    with pytest.raises(_lib.FpmError, match="twice"):           # both lists sorted, id 0 in each
        ops.topk_merge(torch.tensor([[3.0, 2.0, 1.0, 3.0, 2.0, 1.0]]),
                       torch.tensor([[0, 1, 2, 3, 4, 0]], dtype=torch.int32), [0, 3, 6], 2)
    neg = ids.clone()
    neg[0, 0] = -1
    with pytest.raises(_lib.FpmError, match="negative"):
        ok(ids=neg)


# ------------------------------------------------------------------------------------- GalleryIndex.slice
def cpu_index(layout="f32", G=7, labels=None, seed=5):
    """A CPU-device index of G entries with ragged rows and edges (one entry without edges)."""
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(1, 6, (G,), generator=g, dtype=torch.int32)
    cnt = torch.randint(0, 7, (G,), generator=g)
    cnt[1] = 0
    row_off = torch.cat([torch.zeros(1, dtype=torch.int64), n.long().cumsum(0)])
    edge_off = torch.cat([torch.zeros(1, dtype=torch.int64), cnt.cumsum(0)])
    R, E = int(row_off[-1]), int(edge_off[-1])
    y = torch.randn(R, 768, generator=g)
    kw = {} if layout == "f32" else dict(y16=y.to(torch.bfloat16), layout=layout)
    return GalleryIndex(y, row_off, n, torch.randint(0, 5, (E,), generator=g, dtype=torch.int32),
                        torch.randint(0, 5, (E,), generator=g, dtype=torch.int32), torch.rand(E, 2, generator=g),
                        edge_off, torch.rand(G, 512, generator=g), torch.rand(R, 2, generator=g), "f32", 4, "0123abcd",
                        subject=labels, **kw)


def check_slice(part, parent, entries):
    """Every field of ``part`` holds ``parent``'s bytes for ``entries``."""
    ent = entries.tolist()
    assert part.G == len(ent) and part.n.tolist() == parent.n[entries].tolist()
    assert (part.layout, part.sc_mode, part._pack_gen, part.weights_id) == \
        (parent.layout, parent.sc_mode, parent._pack_gen, parent.weights_id)
    assert part.row_off.dtype == torch.int64 and torch.equal(part.row_off.cpu(), part.row_off_host)
    assert (part.y16 is None) == (parent.y16 is None) and (part.P is None) == (parent.P is None)
    assert (part.subject is None) == (parent.subject is None)
    for m, e in enumerate(ent):
        r0, r1 = int(parent.row_off_host[e]), int(parent.row_off_host[e + 1])
        q0, q1 = int(part.row_off_host[m]), int(part.row_off_host[m + 1])
        assert q1 - q0 == r1 - r0
        for name in ("y", "y16", "P"):
            if getattr(parent, name) is not None:
                a, b = getattr(part, name)[q0:q1].cpu(), getattr(parent, name)[r0:r1].cpu()
                assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (name, e)
        e0, e1 = int(parent.edge_off[e]), int(parent.edge_off[e + 1])
        f0, f1 = int(part.edge_off[m]), int(part.edge_off[m + 1])
        assert f1 - f0 == e1 - e0
        for name in ("src", "dst", "pseudo"):
            assert torch.equal(getattr(part, name)[f0:f1].cpu(), getattr(parent, name)[e0:e1].cpu()), (name, e)
        assert torch.equal(part.w[m].cpu(), parent.w[e].cpu())
        if parent.subject is not None:
            assert int(part.subject[m]) == int(parent.subject[e])
    assert int(part.row_off_host[-1]) == part.y.shape[0] and int(part.edge_off[-1]) == part.src.numel()


@pytest.mark.parametrize("layout", ["f32", "f32+bf16", "bf16+host"])
def test_slice_fields_are_the_parents(layout):
    labels = [3, 3, 0, 9, 0, 9, 4]
    parent = cpu_index(layout, labels=labels)
    G = parent.G
    for ent in ([0], [G - 1], [1, 3, 6], list(range(G))):
        entries = torch.tensor(ent, dtype=torch.int64)
        part = parent.slice(entries)
        assert part.device == parent.device
        check_slice(part, parent, entries)
    whole = parent.slice(torch.arange(G))
    assert whole.y.data_ptr() != parent.y.data_ptr()
    assert (whole.nbytes(), whole.host_nbytes()) == (parent.nbytes(), parent.host_nbytes())
    check_slice(cpu_index(layout).slice(torch.tensor([2, 5])), cpu_index(layout), torch.tensor([2, 5]))   # no labels


def test_slice_refusals():
    parent = cpu_index()
    for bad in (torch.tensor([], dtype=torch.int64), torch.tensor([1, 1]), torch.tensor([3, 2]), torch.tensor([-1, 2]),
                torch.tensor([0, 7]), torch.tensor([0, 1], dtype=torch.int32), torch.tensor([[0, 1]])):
        with pytest.raises(_lib.FpmError, match="slice"):
            parent.slice(bad)


# ----------------------------------------------------------------------------------------- ShardedGallery
def check_tables(sg, parent, shard_of):
    G = parent.G
    assert sg.G == G and fpm.ShardedGallery is ShardedGallery
    assert sg.owner.tolist() == shard_of.tolist()
    for s, (part, e) in enumerate(zip(sg.shards, sg.entry)):
        assert e.dtype == torch.int64 and e.tolist() == torch.nonzero(shard_of == s).view(-1).tolist()
        assert sg.local[e].tolist() == list(range(part.G))
        assert sg.entry_d[s].dtype == torch.int32 and sg.entry_d[s].tolist() == e.tolist()
        check_slice(part, parent, e)
    assert sg.n.tolist() == parent.n.tolist()
    assert sg.nbytes() == sum(p.nbytes() for p in sg.shards) and sg.host_nbytes() == parent.host_nbytes()
    assert sg.devices == [torch.device("cpu")] * len(sg.shards) and sg.output_device == torch.device("cpu")


def test_split_tables_for_the_three_assignments():
    labels = [5, 5, 2, 9, 2, 9, 7, 7, 0, 5]
    parent = cpu_index("bf16+host", G=10, labels=labels)
    cpu = torch.device("cpu")
    sg = ShardedGallery.split(parent, [cpu] * 3, "range")
    check_tables(sg, parent, torch.tensor([0, 0, 0, 0, 1, 1, 1, 2, 2, 2]))
    assert sg.subject_split and sg.subject.tolist() == labels and sg.labels.tolist() == [0, 2, 5, 7, 9]
    # whole subjects: subject i of [0, 2, 5, 7, 9] to shard i mod 3
    sg = ShardedGallery.split(parent, [cpu] * 3, "subject")
    shard_of_label = {0: 0, 2: 1, 5: 2, 7: 0, 9: 1}
    check_tables(sg, parent, torch.tensor([shard_of_label[v] for v in labels]))
    assert not sg.subject_split and sg.labels.tolist() == [0, 2, 5, 7, 9]
    assert sg.subject_owner.tolist() == [0, 1, 2, 0, 1] and sg.subject_local.tolist() == [0, 0, 0, 1, 1]
    assert [t.tolist() for t in sg.subject_d] == [[0, 3], [1, 4], [2]]
    assert all(t.dtype == torch.int32 for t in sg.subject_d)
    deal = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0, 1, 1])
    sg = ShardedGallery.split(parent, [cpu] * 2, deal)
    check_tables(sg, parent, deal)
    # the public constructor over sliced parts and explicit tables builds the same tables
    entry = [torch.nonzero(deal == s).view(-1) for s in range(2)]
    again = ShardedGallery([parent.slice(e) for e in entry], entry)
    check_tables(again, parent, deal)
    # default tables: the shards concatenated
    cat = ShardedGallery([parent.slice(torch.arange(0, 4)), parent.slice(torch.arange(4, 10))])
    check_tables(cat, parent, torch.tensor([0] * 4 + [1] * 6))


def test_construction_refusals():
    parent = cpu_index("f32", G=6, labels=[0, 0, 1, 1, 2, 2])
    a, b = parent.slice(torch.tensor([0, 2, 4])), parent.slice(torch.tensor([1, 3, 5]))
    ea, eb = torch.tensor([0, 2, 4]), torch.tensor([1, 3, 5])
    ShardedGallery([a, b], [ea, eb])
    with pytest.raises(_lib.FpmError, match="shards"):
        ShardedGallery([])
    with pytest.raises(_lib.FpmError, match="17 shards"):
        ShardedGallery([a] * 17)
    with pytest.raises(_lib.FpmError, match="GalleryIndex"):
        ShardedGallery([a, "b"])
    with pytest.raises(_lib.FpmError, match="ascend"):
        ShardedGallery([a, b], [torch.tensor([0, 4, 2]), eb])
    with pytest.raises(_lib.FpmError, match="ascend"):
        ShardedGallery([a, b], [torch.tensor([0, 2, 2]), eb])
    with pytest.raises(_lib.FpmError, match="collide"):
        ShardedGallery([a, b], [ea, torch.tensor([1, 2, 5])])
    with pytest.raises(_lib.FpmError, match="ascend|inside"):
        ShardedGallery([a, b], [ea, torch.tensor([1, 3, 6])])
    with pytest.raises(_lib.FpmError, match="entry\\[1\\]"):
        ShardedGallery([a, b], [ea, torch.tensor([1, 3])])
    with pytest.raises(_lib.FpmError, match="int64"):
        ShardedGallery([a, b], [ea, eb.to(torch.int32)])
    with pytest.raises(_lib.FpmError, match="entry tables"):
        ShardedGallery([a, b], [ea])
    other = cpu_index("f32", G=6).slice(torch.tensor([1, 3, 5]))
    with pytest.raises(_lib.FpmError, match="subject labels"):
        ShardedGallery([a, other], [ea, eb])
    bf = cpu_index("f32+bf16", G=6, labels=[0, 0, 1, 1, 2, 2]).slice(eb)
    with pytest.raises(_lib.FpmError, match="layout"):
        ShardedGallery([a, bf], [ea, eb])
    for name, value in (("sc_mode", "bf16"), ("weights_id", "ffff")):
        c = parent.slice(eb)
        setattr(c, name, value)
        with pytest.raises(_lib.FpmError, match=name):
            ShardedGallery([a, c], [ea, eb])
    cpu = torch.device("cpu")
    with pytest.raises(_lib.FpmError, match="without an entry"):
        ShardedGallery.split(parent, [cpu] * 2, torch.zeros(6, dtype=torch.int64))
    with pytest.raises(_lib.FpmError, match="shard number"):
        ShardedGallery.split(parent, [cpu] * 2, torch.tensor([0, 1, 2, 0, 1, 0]))
    with pytest.raises(_lib.FpmError, match="assign"):
        ShardedGallery.split(parent, [cpu] * 2, "hash")
    with pytest.raises(_lib.FpmError, match="subject labels"):
        ShardedGallery.split(cpu_index("f32", G=6), [cpu] * 2, "subject")
    with pytest.raises(_lib.FpmError, match="17 devices"):
        ShardedGallery.split(parent, [cpu] * 17)


def test_probe_set_calls_refuse_a_sharded_gallery():
    parent = cpu_index("f32", G=6)
    sg = ShardedGallery.split(parent, [torch.device("cpu")] * 2)
    net = fpm.Net(regression=True, backbone=False).eval()
    for call in (lambda: net.identify_many(parent, sg, shortlist=2), lambda: net.coarse_scores_many(parent, sg),
                 lambda: net.match_pairs(parent, sg, [[0, 0]])):
        with pytest.raises(_lib.FpmError, match="ShardedGallery"):
            call()
    probe = dict(n=3)
    with pytest.raises(_lib.FpmError, match="shortlist=None"):
        net.identify(probe, sg)
    with pytest.raises(_lib.FpmError, match="select"):
        net.identify(probe, sg, shortlist=2, select=[0, 1])
    with pytest.raises(_lib.FpmError, match="coarse_all"):
        net.identify(probe, parent, coarse_all=False)

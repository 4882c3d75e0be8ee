"""Subject-level 1:N search on the GPU: ``fpm_group_scores`` against its host statement (bit for bit:
both fusions, shared and per-row structures, large rows, composition independence, the C ABI), and
``identify`` / ``identify_many`` with ``by="subject"`` on the planted gallery against the entry-level
calls and the host statement.

The planted gallery (``test_shortlist_gpu.planted``: 40 entries of 24-48 keypoints, the mates of the
three probes at entries 7, 19 and 38) is labelled ``entry // 3``, so the mates fall in subjects 2, 6 and
12 beside two impostor rows each.  The mate's coarse score is 1.54 against at most 0.27 for any other
entry; the max fusion keeps that margin, so the coarse stage must rank the mate's subject
first.  With random weights the exact ranking carries no meaning: no test asserts which subject wins
there, only that every figure is the one the statement gives."""
import ctypes

import pytest
import torch

from fpm import _lib, ops
from fpm.gallery import GalleryIndex
from test_shortlist_cpu import state_dicts
from test_shortlist_gpu import MATES, OUT_KEYS, _net, check_result_keys, planted
from test_subjects_cpu import _bits, _csr, all_cases, cases, per_row_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PAIR_KEYS = tuple(k for k in OUT_KEYS if k not in ("top_idx", "top_score"))
SUBJECT_KEYS = ("subjects", "subject_score", "top_subject", "top_score", "top_idx")
SHORT_KEYS = ("short_subject", "coarse_subject_score", "short_idx", "short_off", "coarse_all")


def _device_groups(s, off, pos, fuse):
    """The kernel's outputs over prefilled buffers (every element must be written)."""
    P, S = s.shape[0], off.shape[-1] - 1
    val = torch.full((P, S), 12345.0, device=DEV)
    best = torch.full((P, S), -7, dtype=torch.int32, device=DEV)
    ops.group_scores(s.to(DEV), off.to(DEV), pos.to(DEV), fuse, gscore=val, gbest=best, off_host=off, pos_host=pos)
    return val.cpu(), best.cpu()


def _same(dev, host):
    return torch.equal(_bits(dev[0]), _bits(host[0])) and torch.equal(dev[1], host[1])


# -------------------------------------------------------------------------- kernel = the statement
@pytest.mark.parametrize("fuse", ops.GROUP_FUSE)
@pytest.mark.parametrize("name", sorted(all_cases()))
def test_kernel_equals_statement(name, fuse):
    s, groups = cases()[name]
    off, pos = _csr(groups)
    host = ops.group_scores(s, off, pos, fuse)
    assert _same(_device_groups(s, off, pos, fuse), host), (name, fuse)
    # a strided device view (row stride > G), as the host case is
    wide = torch.zeros(s.shape[0], s.shape[1] + 9, device=DEV)
    wide[:, 4:4 + s.shape[1]] = s.to(DEV)
    got = ops.group_scores(wide[:, 4:4 + s.shape[1]], off.to(DEV), pos.to(DEV), fuse)
    assert _same((got[0].cpu(), got[1].cpu()), host), (name, fuse)


@pytest.mark.parametrize("fuse", ops.GROUP_FUSE)
def test_kernel_per_row_structures(fuse):
    s, off, pos, shared, other = per_row_case()
    host = ops.group_scores(s, off, pos, fuse)
    dev = _device_groups(s, off, pos, fuse)
    assert _same(dev, host)
    assert torch.equal(_bits(dev[0][0]), _bits(_device_groups(s, *_csr(shared), fuse)[0][0]))


@pytest.mark.parametrize("fuse", ops.GROUP_FUSE)
def test_kernel_large_rows(fuse):
    """3 x 100 000: one group of everything (one wave walks it in team-strided reads) and all singletons."""
    G = 100000
    gen = torch.Generator().manual_seed(12)
    s = torch.randn(3, G, generator=gen)
    one = (torch.tensor([0, G], dtype=torch.int32), torch.randperm(G, generator=gen).to(torch.int32))
    each = (torch.arange(G + 1, dtype=torch.int32), torch.arange(G, dtype=torch.int32))
    for off, pos in (one, each):
        assert _same(_device_groups(s, off, pos, fuse), ops.group_scores(s, off, pos, fuse)), (fuse, off.numel())


def test_kernel_composition_independence():
    """A group's result is the same bits alone (S = 1, P = 1) and inside the full launch, for every count."""
    s, groups = cases()["counts-P3"]
    off, pos = _csr(groups)
    for fuse in ops.GROUP_FUSE:
        full = _device_groups(s, off, pos, fuse)
        for g, members in enumerate(groups):
            alone = _device_groups(s[1:2], *_csr([members]), fuse)
            assert torch.equal(_bits(alone[0][0]), _bits(full[0][1, g:g + 1])), (fuse, g)
            assert int(alone[1][0, 0]) == int(full[1][1, g])


def test_group_scores_c_abi():
    s, groups = cases()["counts-P3"]
    s = s.contiguous()
    off, pos = _csr(groups)
    P_, G, S = s.shape[0], s.shape[1], len(groups)
    lib = _lib.load()
    V = ctypes.c_void_p
    st = V(torch.cuda.current_stream(DEV).cuda_stream)
    s_d, off_d, pos_d = s.to(DEV), off.to(DEV), pos.to(DEV)
    val = torch.full((P_, S), 12345.0, device=DEV)
    best = torch.full((P_, S), -7, dtype=torch.int32, device=DEV)
    args = [V(s_d.data_ptr()), G, P_, G, V(off_d.data_ptr()), 0, V(pos_d.data_ptr()), 0, S, 1, V(val.data_ptr()),
            V(best.data_ptr()), st]
    assert lib.fpm_group_scores(*args) == 0
    assert _same((val.cpu(), best.cpu()), ops.group_scores(s, off, pos, "mean"))
    keep_v, keep_b = val.clone(), best.clone()
    for at, bad, msg in ((9, 2, b"fuse"), (7, 5, b"pos_ld"), (5, S, b"off_ld"), (4, V(0), b"are required"),
                         (2, 70000, b"65535"), (1, G - 1, b"bad sizes"), (8, -1, b"groups")):
        a = list(args)
        a[at] = bad
        assert lib.fpm_group_scores(*a) != 0 and msg in lib.fpm_last_error(), (at, lib.fpm_last_error())
    torch.cuda.synchronize()
    assert torch.equal(_bits(val), _bits(keep_v)) and torch.equal(best, keep_b)      # nothing was launched


# ------------------------------------------------------------------------ the planted gallery, labelled
@pytest.fixture(scope="module")
def sds():
    return state_dicts()


@pytest.fixture(scope="module", params=["f32", "bf16"])
def planted_subjects(request, sds):
    gal, probes = planted()
    net = _net(sds["spread"], request.param)
    labels = [e // 3 for e in range(len(gal))]
    index = net.enroll(gal, DEV, batch=16, subjects=labels)
    return net, probes, gal, index, labels


def _statement_ranking(scores_row, off, labels, entries, fuse, k):
    """subject_score, top_subject, top_score, top_idx by the host statement plus ``rank_topk``."""
    L = int(scores_row.numel())
    gsc, gb = ops.group_scores(scores_row.cpu().view(1, L), off.cpu().to(torch.int32), torch.arange(L, dtype=torch.int32),
                               fuse)
    ti, ts = ops.rank_topk(gsc, k)
    bp = gb[0][ti[0].long()].long()
    te = torch.where(bp >= 0, entries.cpu()[bp.clamp(min=0)], torch.full_like(bp, -1).to(torch.int32))
    return gsc[0], labels.cpu()[ti[0].long()], ts[0], te


def _check_subject_ranking(r, fuse, k, score="cls_prob"):
    gsc, tl, ts, te = _statement_ranking(r[score].view(-1), r["short_off"], r["subjects"], r["short_idx"], fuse, k)
    assert torch.equal(_bits(r["subject_score"].cpu()), _bits(gsc))
    assert r["top_subject"].dtype == torch.int64 and torch.equal(r["top_subject"].cpu(), tl)
    assert torch.equal(_bits(r["top_score"].cpu()), _bits(ts))
    assert r["top_idx"].dtype == torch.int32 and torch.equal(r["top_idx"].cpu(), te.to(torch.int32))


def test_enrolment_with_labels_changes_nothing_else(planted_subjects):
    net, probes, gal, index, labels = planted_subjects
    plain = net.enroll(gal, DEV, batch=16)
    assert plain.subject is None and index.subject.tolist() == labels and index.subject.device.type == "cpu"
    for k in ("y", "row_off", "n", "src", "dst", "pseudo", "edge_off", "w", "P"):
        assert torch.equal(getattr(plain, k), getattr(index, k)), k
    assert (plain.layout, plain.sc_mode, plain.weights_id) == (index.layout, index.sc_mode, index.weights_id)


@pytest.mark.parametrize("impressions", ["all", "best"])
def test_shortlisted_subject_identify(planted_subjects, impressions):
    net, probes, gal, index, labels = planted_subjects
    gt = index.subject_groups()
    for fuse in ops.GROUP_FUSE:
        res = net.identify(probes, index, topk=4, shortlist=4, by="subject", fuse=fuse, impressions=impressions)
        for p, r in enumerate(res):
            mate = [e for e, q in MATES.items() if q == p][0]
            # coarse stage: the statement on coarse_all (max whatever fuse is), the mate's subject first
            call = r["coarse_all"].cpu().view(1, -1)
            cg, cb = ops.group_scores(call, gt["off"], gt["pos"], "max")
            hi, hs = ops.rank_select(cg, 4)
            assert r["short_subject"].dtype == torch.int64
            assert torch.equal(r["short_subject"].cpu(), gt["labels"][hi[0].long()])
            assert torch.equal(_bits(r["coarse_subject_score"].cpu()), _bits(hs[0]))
            assert int(r["short_subject"][0]) == mate // 3
            assert torch.equal(_bits(r["coarse_all"]), _bits(net.coarse_scores(probes[p], index)[0]))
            # the entry list: subject-major in coarse-rank order
            want, woff = [], [0]
            for s in hi[0].tolist():
                members = [e for e in range(len(gal)) if labels[e] == int(gt["labels"][s])]
                want += members if impressions == "all" else [int(cb[0, s])]
                woff.append(len(want))
            assert r["short_idx"].dtype == torch.int32 and r["short_idx"].tolist() == want
            assert r["short_off"].tolist() == woff
            if impressions == "best":
                assert mate in want
            # exact stage: the entry-level identify over exactly those entries, bit for bit
            ref = net.identify(probes[p], index, topk=4, select=r["short_idx"])
            check_result_keys(r, "identify", "subject", True, k=4, M=4, S=4, L=len(want), Gs=len(gal))
            for k in PAIR_KEYS:
                assert r[k].dtype == ref[k].dtype and torch.equal(r[k], ref[k]), (fuse, p, k)
            assert torch.equal(r["subjects"], r["short_subject"])
            _check_subject_ranking(r, fuse, 4)


def test_by_none_is_unchanged_and_full_query_by_subject(planted_subjects):
    net, probes, gal, index, labels = planted_subjects
    probe = probes[1]
    new = set(SUBJECT_KEYS + SHORT_KEYS + ("short_off",)) - {"top_score", "top_idx", "short_idx", "coarse_all"}
    sel = [30, 7, 19, 6, 8, 39, 18, 0, 20, 31, 5]
    plain = net.identify(probe, index, topk=5, select=sel)
    short = net.identify(probe, index, topk=3, shortlist=3)
    assert not new & set(plain) and not new & set(short)
    check_result_keys(plain, "identify", None, False, k=5)
    check_result_keys(short, "identify", None, True, k=3, M=3, Gs=len(gal))
    gt = index.subject_groups(sel)
    for fuse in ops.GROUP_FUSE:
        r = net.identify(probe, index, topk=5, select=sel, by="subject", fuse=fuse)
        assert set(r) == set(plain) | set(SUBJECT_KEYS)
        check_result_keys(r, "identify", "subject", False, k=5, S=len(gt["labels"]))
        for k in PAIR_KEYS:
            assert torch.equal(r[k], plain[k]), k
        assert r["subjects"].dtype == torch.int64 and r["subjects"].tolist() == sorted({labels[e] for e in sel})
        gsc, gb = ops.group_scores(plain["cls_prob"].cpu().view(1, -1), gt["off"], gt["pos"], fuse)
        ti, ts = ops.rank_topk(gsc, 5)
        assert torch.equal(_bits(r["subject_score"].cpu()), _bits(gsc[0]))
        assert torch.equal(r["top_subject"].cpu(), gt["labels"][ti[0].long()])
        assert torch.equal(_bits(r["top_score"].cpu()), _bits(ts[0]))
        assert r["top_idx"].tolist() == [sel[int(gb[0, s])] for s in ti[0].tolist()]
    # more ranks asked for than there are subjects: k is clamped to S
    assert tuple(net.identify(probe, index, topk=50, select=sel, by="subject")["top_subject"].shape) == (len(gt["labels"]),)


def test_identify_many_by_subject(planted_subjects):
    """A probe set against the one-probe calls.  With every probe a group of its own the padded boxes are
    the one-probe calls', and every output is their bits.  In one group the coarse stage and the entry
    lists are still the one-probe calls' bits; the exact stage runs in the group's box, so (as for the
    entry-level ``identify_many``) its outputs are held to ``match_pairs`` over the group's pair list and
    to the statement's ranking of those scores."""
    net, probes, gal, index, labels = planted_subjects
    pset = net.enroll(probes, DEV, batch=2)
    kw = dict(topk=4, shortlist=4, by="subject", fuse="mean", impressions="all")
    one = net.identify(probes, index, **kw)
    alone = net.identify_many(pset, index, group_pairs=12, **kw)
    assert sorted(r["group"][0] for r in alone) == [0, 1, 2]
    for p, (a, b) in enumerate(zip(alone, one)):
        L = int(b["short_off"][-1])                          # the impressions of the four shortlisted subjects
        check_result_keys(a, "identify_many", "subject", True, k=4, M=4, S=4, L=L, Gs=len(gal))
        check_result_keys(b, "identify", "subject", True, k=4, M=4, S=4, L=L, Gs=len(gal))
        for k in PAIR_KEYS + SUBJECT_KEYS + SHORT_KEYS:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (p, k)
        for k in ("subject_score", "top_score", "coarse_subject_score", "coarse_all"):
            assert torch.equal(_bits(a[k]), _bits(b[k])), (p, k)
    together = net.identify_many(pset, index, **kw)
    assert [r["group"][0] for r in together] == [0, 0, 0]
    order = sorted(range(3), key=lambda p: together[p]["group"][1])
    pairs = [(p, e) for p in order for e in together[p]["short_idx"].tolist()]
    ref = net.match_pairs(pset, index, pairs)
    for p, (a, b) in enumerate(zip(together, one)):
        for k in SHORT_KEYS:
            assert torch.equal(a[k], b[k]), (p, k)
        for k in ("coarse_subject_score", "coarse_all"):
            assert torch.equal(_bits(a[k]), _bits(b[k])), (p, k)
        _, b0, b1 = a["group"]
        assert b1 - b0 == int(a["short_idx"].numel())
        for k in ("s", "ss", "ds_mat", "perm_mat", "k_prob", "cls_prob"):
            assert torch.equal(a[k], ref[k][b0:b1]), (p, k)
        _check_subject_ranking(a, "mean", 4)
        print("MEASURE identify_many one group, probe %d: exact scores %s the one-probe call's bits"
              % (p, "are" if torch.equal(_bits(a["cls_prob"]), _bits(b["cls_prob"])) else "are not"))
    # impressions="best" and the max: four pairs per probe, again a group each
    kw.update(fuse="max", impressions="best")
    best = net.identify_many(pset, index, group_pairs=4, **kw)
    for a, b in zip(best, net.identify(probes, index, **kw)):
        check_result_keys(a, "identify_many", "subject", True, k=4, M=4, S=4, L=4, Gs=len(gal))
        for k in PAIR_KEYS + SUBJECT_KEYS + SHORT_KEYS:
            assert torch.equal(a[k], b[k]), k
    # without a shortlist the probe-set query still carries its ragged pair lists (short_idx / short_off): every
    # entry, subject-major; the one-probe query (test_by_none_is_unchanged_and_full_query_by_subject) does not
    S = len(set(labels))
    for r in net.identify_many(pset, index, topk=4, by="subject", fuse="mean"):
        check_result_keys(r, "identify_many", "subject", False, k=4, S=S, L=len(gal))
        assert sorted(r["short_idx"].tolist()) == list(range(len(gal))) and int(r["short_off"][-1]) == len(gal)
        _check_subject_ranking(r, "mean", 4)


def test_leave_one_out(planted_subjects):
    net, probes, gal, index, _ = planted_subjects
    sel = [7, 3, 19, 12, 38, 25, 30, 5, 33]
    subject = {7: 100, 3: 100, 19: 100, 12: 100, 38: 200, 25: 200, 30: 200, 5: 200, 33: 300}
    labels = [subject.get(e, 1000 + e) for e in range(len(gal))]
    twin = GalleryIndex(index.y, index.row_off, index.n, index.src, index.dst, index.pseudo, index.edge_off, index.w,
                        index.P, index.sc_mode, index._pack_gen, index.weights_id, subject=labels)
    for impressions in ("all", "best"):
        res = net.identify_many(twin, twin, topk=3, shortlist=3, select=sel, probe_select=sel, exclude_self=True,
                                by="subject", fuse="mean", impressions=impressions)
        assert len(res) == len(sel)
        for q, r in zip(sel, res):
            short = r["short_idx"].tolist()
            assert q not in short and q not in r["top_idx"].tolist()
            assert sorted(r["short_subject"].tolist()) == [100, 200, 300]
            mates = [e for e in sel if subject[e] == subject[q] and e != q]
            at = r["short_subject"].tolist().index(subject[q])
            mine = short[int(r["short_off"][at]):int(r["short_off"][at + 1])]
            if impressions == "all":
                assert sorted(short) == sorted(e for e in sel if e != q) and sorted(mine) == sorted(mates)
            else:
                assert len(mine) == min(1, len(mates)) and set(mine) <= set(mates)
            # the coarse fuse saw the probe's own entry as -inf
            masked = r["coarse_all"].cpu().clone().view(1, -1)
            masked[0, sel.index(q)] = float("-inf")
            gt = twin.subject_groups(sel)
            hi, hs = ops.rank_select(ops.group_scores(masked, gt["off"], gt["pos"], "max")[0], 3)
            assert torch.equal(r["short_subject"].cpu(), gt["labels"][hi[0].long()])
            assert torch.equal(_bits(r["coarse_subject_score"].cpu()), _bits(hs[0]))
            _check_subject_ranking(r, "mean", 3)
            if q == 33:
                # the singleton subject emptied by the exclusion: last in both stages, NaN, no entry
                assert int(r["short_subject"][2]) == 300 and float(r["coarse_subject_score"][2]) == float("-inf")
                assert int(r["top_subject"][2]) == 300 and bool(torch.isnan(r["top_score"][2]))
                assert int(r["top_idx"][2]) == -1 and bool(torch.isfinite(r["top_score"][:2]).all())
            else:
                assert bool(torch.isfinite(r["subject_score"][r["short_subject"] != 300]).all())


def test_host_row_layout_agrees(planted_subjects):
    net, probes, gal, index, labels = planted_subjects
    host = net.enroll(gal, DEV, batch=16, layout="bf16+host", subjects=labels)
    kw = dict(topk=4, shortlist=4, by="subject", fuse="mean", impressions="all")
    a, b = net.identify(probes[0], host, **kw), net.identify(probes[0], index, **kw)
    assert set(a) == set(b)
    for k in PAIR_KEYS + SUBJECT_KEYS + SHORT_KEYS:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    for k in ("subject_score", "top_score", "coarse_subject_score", "coarse_all"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k

"""Open-set 1:N search on the GPU: ``fpm_group_topr`` and ``fpm_cohort_decide`` against their host statements
(bit for bit: every case of the CPU tests, the whole-wave path, teams of unequal counts side by side in one wave,
row counts that are no multiple of the rows per workgroup, the edge rows, the C ABI), and ``identify`` /
``identify_many`` with the open-set keywords on the planted gallery of ``test_shortlist_gpu`` (40 entries, three
probes, labels ``entry // 3``, f32 and bf16 nets): every key a call returns without the new arguments is the same
bits with them, and every new key is the CPU statement applied to the call's own returned score rows.

With random weights the exact scores carry no meaning: no threshold value, separation margin or timing is asserted,
only that every figure is the one the statements give."""
import ctypes

import pytest
import torch

from fpm import _lib, ops
from fpm.gallery import GalleryIndex
from test_open_set_cpu import INF, NAN, QNAN, _ubits, edge_rows, ranked_rows
from test_shortlist_cpu import state_dicts
from test_shortlist_gpu import _net, planted
from test_subjects_cpu import _bits, _csr, all_cases, cases, per_row_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KERNEL_RS = (1, 2, 16)


def _device_topr(s, off, pos, r):
    """The kernel's outputs over prefilled buffers (every element must be written)."""
    P, S = s.shape[0], off.shape[-1] - 1
    val = torch.full((P, S), 12345.0, device=DEV)
    best = torch.full((P, S), -7, dtype=torch.int32, device=DEV)
    ops.group_topr(s.to(DEV), off.to(DEV), pos.to(DEV), r, gscore=val, gbest=best, off_host=off, pos_host=pos)
    return val.cpu(), best.cpu()


def _same(dev, host):
    return torch.equal(_bits(dev[0]), _bits(host[0])) and torch.equal(dev[1], host[1])


# ------------------------------------------------------------------------- group_topr: kernel = statement
@pytest.mark.parametrize("r", KERNEL_RS)
@pytest.mark.parametrize("name", sorted(all_cases()))
def test_topr_kernel_equals_statement(name, r):
    s, groups = cases()[name]                                # "one-group": 5000 entries, the whole-wave path
    off, pos = _csr(groups)
    host = ops.group_topr(s, off, pos, r)
    assert _same(_device_topr(s, off, pos, r), host), (name, r)
    # a strided device view (row stride > G), as the host case is
    wide = torch.zeros(s.shape[0], s.shape[1] + 9, device=DEV)
    wide[:, 4:4 + s.shape[1]] = s.to(DEV)
    got = ops.group_topr(wide[:, 4:4 + s.shape[1]], off.to(DEV), pos.to(DEV), r)
    assert _same((got[0].cpu(), got[1].cpu()), host), (name, r)


@pytest.mark.parametrize("r", KERNEL_RS)
def test_topr_kernel_per_row_structures(r):
    s, off, pos, shared, other = per_row_case()
    dev = _device_topr(s, off, pos, r)
    assert _same(dev, ops.group_topr(s, off, pos, r))
    assert torch.equal(_bits(dev[0][0]), _bits(_device_topr(s, *_csr(shared), r)[0][0]))


@pytest.mark.parametrize("r", KERNEL_RS)
def test_topr_kernel_unequal_teams_and_a_wide_group(r):
    """Counts 0, 1, 15, 16 and 17 cycling over 70 groups: the four teams of every wave hold different counts (and
    run out in different rounds), yet every lane reaches every shuffle of all r rounds.  A group of 5000 in the
    second tile takes the whole-wave pass beside them.  NaN, infinities, ties and repeated positions are mixed in."""
    gen = torch.Generator().manual_seed(41)
    G = 6000
    s = (torch.randn(3, G, generator=gen) * 2).round() / 2
    s[0, ::7] = NAN
    s[1, ::11] = INF
    s[2, ::5] = -INF
    groups, at = [], 0
    perm = torch.randperm(G, generator=gen).tolist()
    for i in range(70):
        c = (0, 1, 15, 16, 17)[i % 5]
        groups.append(perm[at:at + c])
        at += c
    groups[66] = perm[:5000]
    groups[3] = groups[3][:8] + groups[3][:8]                # positions twice in one group
    off, pos = _csr(groups)
    assert _same(_device_topr(s, off, pos, r), ops.group_topr(s, off, pos, r))


def test_topr_kernel_composition_independence():
    s, groups = cases()["counts-P3"]
    off, pos = _csr(groups)
    for r in (2, 16):
        full = _device_topr(s, off, pos, r)
        for g, members in enumerate(groups):
            alone = _device_topr(s[1:2], *_csr([members]), r)
            assert torch.equal(_bits(alone[0][0]), _bits(full[0][1, g:g + 1])), (r, g)
            assert int(alone[1][0, 0]) == int(full[1][1, g])


# ---------------------------------------------------------------------- cohort_decide: kernel = statement
def _same_cohort(dev, host):
    for d, h in zip(dev, host):
        assert (d is None) == (h is None)
        if d is not None and not (d.dtype == h.dtype and d.shape == h.shape and torch.equal(_bits(d.cpu()), _bits(h))):
            return False
    return True


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 130, 1024])
def test_cohort_kernel_equals_statement(K):
    for P in (1, 3, 5):                                      # not a multiple of the four rows per workgroup
        top = ranked_rows(P, K, 50 + K + P)
        top[P - 1, K * 2 // 3 + (K == 1):] = NAN             # the last row: a NaN tail
        top_d = top.to(DEV)
        for skip in (0, 1, 5):
            for cohort in (2, 31, 64, 1019):
                for k, thr, norm in ((1, None, True), (min(K, 70), 0.5, True), (K, 0.5, False)):
                    host = ops.cohort_decide(top, k, skip, cohort, 1e-6, thr, norm)
                    dev = ops.cohort_decide(top_d, k, skip, cohort, 1e-6, thr, norm)
                    assert _same_cohort(dev, host), (P, K, skip, cohort, k, thr, norm)


def test_cohort_kernel_edge_rows():
    top, what = edge_rows()
    top_d = top.to(DEV)
    for kw in (dict(threshold=3.0), dict(threshold=-INF), dict(threshold=INF), dict(sigma_floor=0.5, threshold=14.0),
               dict(threshold=4.0, normalize=False), dict()):
        assert _same_cohort(ops.cohort_decide(top_d, 3, 1, 4, **kw), ops.cohort_decide(top, 3, 1, 4, **kw)), kw
    for K, skip in ((1, 1), (3, 3), (3, 7)):                 # the window past the row's end: n = 0
        cut = top[:, :K].contiguous()
        dev = ops.cohort_decide(cut.to(DEV), 1, skip, 4, threshold=-INF)
        assert _same_cohort(dev, ops.cohort_decide(cut, 1, skip, 4, threshold=-INF)) and dev[3].tolist() == [0] * 10
    # rows that are not sorted (NaN in the middle of the window): the cohort is still the non-NaN values in order
    mixed = ranked_rows(6, 200, 77)
    mixed[:, 3::4] = NAN
    assert _same_cohort(ops.cohort_decide(mixed.to(DEV), 9, 2, 150, threshold=0.0), ops.cohort_decide(mixed, 9, 2, 150, threshold=0.0))


# ------------------------------------------------------------------------------------------- the C ABI
def test_group_topr_c_abi():
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
    args = [V(s_d.data_ptr()), G, P_, G, V(off_d.data_ptr()), 0, V(pos_d.data_ptr()), 0, S, 3, V(val.data_ptr()),
            V(best.data_ptr()), st]
    assert lib.fpm_group_topr(*args) == 0
    assert _same((val.cpu(), best.cpu()), ops.group_topr(s, off, pos, 3))
    keep_v, keep_b = val.clone(), best.clone()
    for at, bad, msg in ((9, 0, b"r = 0"), (9, 17, b"r = 17"), (7, 5, b"pos_ld"), (5, S, b"off_ld"), (4, V(0), b"are required"),
                         (10, V(0), b"are required"), (2, 70000, b"65535"), (1, G - 1, b"bad sizes"), (8, -1, b"groups")):
        a = list(args)
        a[at] = bad
        assert lib.fpm_group_topr(*a) != 0 and msg in lib.fpm_last_error(), (at, lib.fpm_last_error())
    torch.cuda.synchronize()
    assert torch.equal(_bits(val), _bits(keep_v)) and torch.equal(best, keep_b)      # nothing was launched


def test_cohort_decide_c_abi():
    top = ranked_rows(5, 40, 9)
    P_, K, k = 5, 40, 6
    lib = _lib.load()
    V = ctypes.c_void_p
    st = V(torch.cuda.current_stream(DEV).cuda_stream)
    top_d = top.to(DEV)
    z = torch.full((P_, k), 12345.0, device=DEV)
    mu, sigma = torch.full((P_,), 12345.0, device=DEV), torch.full((P_,), 12345.0, device=DEV)
    n = torch.full((P_,), -7, dtype=torch.int32, device=DEV)
    acc = torch.full((P_, k), -7, dtype=torch.int32, device=DEV)
    outs = (z, mu, sigma, n, acc)
    args = [V(top_d.data_ptr()), P_, K, k, 1, 32, 1e-6, 1, 1, 1.0] + [V(t.data_ptr()) for t in outs] + [st]
    assert lib.fpm_cohort_decide(*args) == 0
    assert _same_cohort(outs, ops.cohort_decide(top, k, 1, 32, 1e-6, 1.0))
    keep = [t.clone() for t in outs]
    for at, bad, msg in ((3, 0, b"bad sizes"), (3, 41, b"bad sizes"), (2, 0, b"bad sizes"), (4, -1, b"skip = -1"),
                         (5, 1, b"cohort = 1"), (5, 1024, b"skip + cohort <= 1024"), (6, 0.0, b"sigma_floor"),
                         (6, INF, b"sigma_floor"), (6, NAN, b"sigma_floor"), (9, NAN, b"threshold is NaN"),
                         (7, 2, b"normalize = 2"), (0, V(0), b"top is required"), (10, V(0), b"top is required"),
                         (13, V(0), b"top is required"), (14, V(0), b"top is required"), (1, 70000, b"65535")):
        a = list(args)
        a[at] = bad
        assert lib.fpm_cohort_decide(*a) != 0 and msg in lib.fpm_last_error(), (at, lib.fpm_last_error())
    a = list(args)
    a[7] = a[8] = 0
    assert lib.fpm_cohort_decide(*a) != 0 and b"not both 0" in lib.fpm_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(t), _bits(kept)) for t, kept in zip(outs, keep))       # nothing was launched
    # the parts not asked for may be null
    a = list(args)
    a[7] = 0
    a[10:14] = [V(0)] * 4
    assert lib.fpm_cohort_decide(*a) == 0
    assert torch.equal(acc.cpu(), ops.cohort_decide(top, k, threshold=1.0, normalize=False)[4])
    assert all(torch.equal(_bits(t), _bits(kept)) for t, kept in zip(outs[:4], keep[:4]))


# ------------------------------------------------------------------------ the planted gallery, end to end
OPEN = dict(normalize="cohort", cohort=4, cohort_skip=1)
Z_KEYS = {"top_z", "cohort_mu", "cohort_sigma", "cohort_n"}
DECISION_KEYS = {"accept", "match"}


@pytest.fixture(scope="module")
def sds():
    return state_dicts()


@pytest.fixture(scope="module", params=["f32", "bf16"])
def planted_open(request, sds):
    gal, probes = planted()
    net = _net(sds["spread"], request.param)
    labels = [e // 3 for e in range(len(gal))]
    index = net.enroll(gal, DEV, batch=16, subjects=labels)
    return net, probes, index, labels


def _ranked_row(r, by):
    """The row a result's ranking ranked, from the result itself: the fused subject scores, or the exact scores."""
    return (r["subject_score"] if by else r["cls_prob"]).detach().cpu().view(1, -1)


def _check_open_keys(r, base, by, k, threshold, normalize=True, cohort=4, skip=1):
    """``r`` (a result with the open-set keywords) against ``base`` (the same call without them) and the CPU
    statements applied to r's own score row."""
    added = (Z_KEYS if normalize else set()) | (DECISION_KEYS if threshold is not None else set())
    assert set(r) == set(base) | added and not added & set(base)
    for key, v in base.items():
        if not isinstance(v, torch.Tensor):
            assert r[key] == v, key
        elif v.dtype == torch.float32:                       # bits: NaN scores (an emptied subject) compare too
            assert r[key].dtype == v.dtype and r[key].shape == v.shape and torch.equal(_bits(r[key]), _bits(v)), key
        else:
            assert r[key].dtype == v.dtype and torch.equal(r[key], v), key
    row = _ranked_row(r, by)
    K = min(row.shape[1], max(k, skip + cohort))
    _, top = ops.rank_select(row, K)
    assert torch.equal(_bits(top[0, :k]), _bits(r["top_score"].cpu()))
    z, mu, sigma, n, acc = ops.cohort_decide(top, k, skip, cohort, 1e-6, threshold, normalize)
    if normalize:
        assert r["top_z"].dtype == torch.float32 and tuple(r["top_z"].shape) == (k,) and r["top_z"].device == DEV
        assert torch.equal(_bits(r["top_z"].cpu()), _bits(z[0]))
        for key, want, dt in (("cohort_mu", mu, torch.float32), ("cohort_sigma", sigma, torch.float32), ("cohort_n", n, torch.int32)):
            assert r[key].dtype == dt and r[key].dim() == 0 and int(_bits(r[key].cpu())) == int(_bits(want)[0]), key
    if threshold is not None:
        assert r["accept"].dtype == torch.bool and r["accept"].tolist() == [bool(a) for a in acc[0]]
        first = int(r["top_subject"][0]) if by else int(r["top_idx"][0])
        assert r["match"].dtype == torch.int64 and r["match"].dim() == 0
        assert int(r["match"]) == (first if bool(acc[0, 0]) else -1)


def _both_infinities(call, base, by, k):
    """threshold -inf with the z-scores: every non-NaN z is accepted; +inf on the raw scores: none, match -1."""
    for r, b in zip(call(threshold=-INF, **OPEN), base):
        _check_open_keys(r, b, by, k, -INF)
        assert r["accept"].tolist() == (~torch.isnan(r["top_z"])).tolist() and bool(r["accept"][0])
        assert int(r["match"]) == (int(r["top_subject"][0]) if by else int(r["top_idx"][0]))
    for r, b in zip(call(threshold=INF), base):
        _check_open_keys(r, b, by, k, INF, normalize=False)
        assert not bool(r["accept"].any()) and int(r["match"]) == -1


@pytest.mark.parametrize("by", [None, "subject"])
@pytest.mark.parametrize("shortlist", [None, 8])
def test_identify_open_set(planted_open, shortlist, by):
    net, probes, index, labels = planted_open
    kw = dict(topk=5, shortlist=shortlist, by=by)
    if by:
        kw.update(fuse="mean")
    base = net.identify(probes, index, **kw)
    _both_infinities(lambda **o: net.identify(probes, index, **kw, **o), base, by, 5)
    one = net.identify(probes[1], index, threshold=0.5, **kw, **OPEN)      # one probe: a dict, 0-d statistics
    _check_open_keys(one, base[1], by, 5, 0.5)


@pytest.mark.parametrize("by", [None, "subject"])
@pytest.mark.parametrize("shortlist", [None, 8])
def test_identify_many_open_set(planted_open, shortlist, by):
    net, probes, index, labels = planted_open
    pset = net.enroll(probes, DEV, batch=2)
    kw = dict(topk=5, shortlist=shortlist, by=by)
    if by:
        kw.update(fuse="mean")
    base = net.identify_many(pset, index, **kw)
    _both_infinities(lambda **o: net.identify_many(pset, index, **kw, **o), base, by, 5)


@pytest.mark.parametrize("top_r", [1, 2, 3])
def test_top_r_is_the_statement_on_the_exact_rows(planted_open, top_r):
    net, probes, index, labels = planted_open
    kw = dict(topk=4, by="subject", fuse="mean", top_r=top_r)
    plain = net.identify(probes, index, topk=4, by="subject", fuse="mean")
    gt = index.subject_groups()
    for r, b in zip(net.identify(probes, index, **kw), plain):                   # every entry: the selection's groups
        assert set(r) == set(b)
        gsc, gb = ops.group_topr(r["cls_prob"].cpu().view(1, -1), gt["off"], gt["pos"], top_r)
        ti, ts = ops.rank_topk(gsc, 4)
        assert torch.equal(_bits(r["subject_score"].cpu()), _bits(gsc[0])) and torch.equal(_bits(r["top_score"].cpu()), _bits(ts[0]))
        assert torch.equal(r["top_subject"].cpu(), gt["labels"][ti[0].long()])
        assert r["top_idx"].tolist() == [int(gb[0, s]) for s in ti[0].tolist()]
        for key in ("cls_prob", "s", "perm_mat"):
            assert torch.equal(r[key], b[key]), key
    short = dict(shortlist=4, threshold=0.0, **kw, **OPEN)
    pset = net.enroll(probes, DEV, batch=2)
    one = net.identify(probes, index, **short)
    for res in (one, net.identify_many(pset, index, **short)):
        for r in res:                                                            # shortlisted: the ragged lists
            L = int(r["short_idx"].numel())
            gsc, gb = ops.group_topr(r["cls_prob"].cpu().view(1, L), r["short_off"].cpu(), torch.arange(L, dtype=torch.int32), top_r)
            assert torch.equal(_bits(r["subject_score"].cpu()), _bits(gsc[0]))
            ti, ts = ops.rank_topk(gsc, 4)
            assert torch.equal(_bits(r["top_score"].cpu()), _bits(ts[0]))
            assert r["top_idx"].tolist() == [int(r["short_idx"][int(gb[0, s])]) for s in ti[0].tolist()]
            _, top = ops.rank_select(gsc, 4)
            z = ops.cohort_decide(top, 4, 1, 4, 1e-6, 0.0)
            assert torch.equal(_bits(r["top_z"].cpu()), _bits(z[0][0])) and r["accept"].tolist() == [bool(a) for a in z[4][0]]
    # the coarse stage keeps fusing by max: the shortlist is the plain call's
    for r, b in zip(one, net.identify(probes, index, topk=4, by="subject", fuse="mean", shortlist=4)):
        assert torch.equal(r["short_subject"], b["short_subject"]) and torch.equal(r["short_idx"], b["short_idx"])


@pytest.mark.parametrize("by", [None, "subject"])
def test_leave_one_out_open_set(planted_open, by):
    """``exclude_self``: at entry level the probe's own entry is in no list; at subject level the singleton subject
    emptied by the exclusion has a NaN score: it ranks last, its z is NaN, it is not accepted and it is outside
    every cohort (``cohort_n`` counts the two others)."""
    net, probes, index, _ = planted_open
    sel = [7, 3, 19, 12, 38, 25, 30, 5, 33]
    subject = {7: 100, 3: 100, 19: 100, 12: 100, 38: 200, 25: 200, 30: 200, 5: 200, 33: 300}
    labels = [subject.get(e, 1000 + e) for e in range(index.G)]
    twin = GalleryIndex(index.y, index.row_off, index.n, index.src, index.dst, index.pseudo, index.edge_off, index.w,
                        index.P, index.sc_mode, index._pack_gen, index.weights_id, subject=labels)
    kw = dict(topk=3, shortlist=3 if by else 5, select=sel, probe_select=sel, exclude_self=True, by=by)
    opts = dict(normalize="cohort", cohort=3, cohort_skip=0, threshold=-INF)
    if by:
        kw.update(fuse="mean", top_r=2)
    base = net.identify_many(twin, twin, **kw)
    res = net.identify_many(twin, twin, **kw, **opts)
    for q, r, b in zip(sel, res, base):
        _check_open_keys(r, b, by, 3, -INF, cohort=3, skip=0)
        assert q not in r["short_idx"].tolist()
        if by and q == 33:
            assert int(r["top_subject"][2]) == 300 and bool(torch.isnan(r["top_score"][2]))
            assert int(_ubits(r["top_z"].cpu())[2]) == QNAN and r["accept"].tolist() == [True, True, False]
            assert int(r["cohort_n"]) == 2
        else:
            assert int(r["cohort_n"]) == 3 and r["accept"].tolist() == [True] * 3

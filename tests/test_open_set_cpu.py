"""Open-set 1:N search, host side (no GPU): the statements of ``ops.group_topr`` and ``ops.cohort_decide`` against
independent plain definitions (per-group and per-row Python loops in numpy fp32: equal bits), against float64, on
the edge rows, every refusal of the two wrappers and of the query layer's new keywords, and the query layer's one
open-set stage (``gallery._open_set``) on CPU tensors against the composition of ``rank_select`` and the statement.

Bounds against float64 (from the arithmetic, not from what the code gives):
  top-r   r' - 1 effective sequential additions and one division, each within 2^-24 relative of a partial sum of at
          most r' max|x|: |gscore - mean64| <= r' 2^-23 max|x| over all-finite groups (the worst seen was 0.23 of it).
  cohort  |mu - mu64| and |sigma - sigma64| <= n 2^-23 max|x| on rows with sigma64 >= 0.05 max|x| (where the square
          root does not amplify the sum's error), n from 2 to 1023 (the worst seen was 0.21 of it).
"""
import math
import types

import numpy as np
import pytest
import torch

from fpm import _lib, gallery, ops
from test_compact_index_cpu import hand_index
from test_subjects_cpu import _bits, _csr, all_cases, per_row_case

RS = (1, 2, 3, 8, 16)
QNAN = 0x7FC00000
F = np.float32
NAN, INF = float("nan"), float("inf")

_CASES = {}


def cases():
    if not _CASES:
        _CASES.update(all_cases())
    return _CASES


def _ubits(t):
    """A tensor's fp32 (or int32) bit patterns as non-negative integers."""
    return _bits(t).to(torch.int64) & 0xFFFFFFFF


def _f32bits(v):
    v = F(v)
    return QNAN if np.isnan(v) else int(v.view(np.uint32))


def _order(row, members):
    """A group's entries best first: score descending (+0.0 before -0.0, as ``rank_key`` has it), NaN last,
    then position ascending."""
    def key(q):
        x = float(row[q])
        return (math.isnan(x), 0.0 if math.isnan(x) else -x, math.copysign(1.0, x) < 0, q)
    return sorted(members, key=key)


def plain_topr(row, members, r, order=None):
    """The plain definition of one group -> (gscore bits, gbest); ``row``: numpy fp32."""
    if not members:
        return QNAN, -1
    order = _order(row, members) if order is None else order
    rp = min(r, len(members))
    s = F(0.0)
    with np.errstate(all="ignore"):
        for q in order[:rp]:
            s = F(s + row[q])
        return _f32bits(s / F(rp)), order[0]


def plain_lane_sum(v):
    lanes = [F(0.0)] * 64
    with np.errstate(all="ignore"):
        for j, a in enumerate(v):
            lanes[j % 64] = F(lanes[j % 64] + a)
        m = 32
        while m:
            lanes = [F(lanes[t] + lanes[t ^ m]) for t in range(64)]
            m //= 2
    return lanes[0]


def plain_cohort(row, k, skip, cohort, floor=1e-6):
    """The plain definition of one row -> (z bits (k), mu bits, sigma bits, n); ``row``: numpy fp32 (K,)."""
    x = [v for v in row[skip:min(len(row), skip + cohort)] if not np.isnan(v)]
    n = len(x)
    mu = sigma = F(NAN)
    with np.errstate(all="ignore"):
        if n >= 2:
            mu = F(plain_lane_sum(x) / F(n))
            d = [F(v - mu) for v in x]
            sigma = F(np.sqrt(F(plain_lane_sum([F(a * a) for a in d]) / F(n))))
        s = F(NAN) if np.isnan(sigma) else max(sigma, F(floor))
        z = [_f32bits(F(F(row[j] - mu) / s)) for j in range(k)]
    return z, _f32bits(mu), _f32bits(sigma), n


def check_cohort(top, k, skip, cohort, floor=1e-6, got=None):
    """``got`` (default: the statement on ``top``) against the plain definition, row by row, bit for bit."""
    z, mu, sigma, n, _ = ops.cohort_decide(top, k, skip, cohort, floor) if got is None else got
    assert z.dtype == torch.float32 and tuple(z.shape) == (top.shape[0], k) and n.dtype == torch.int32
    for p in range(top.shape[0]):
        wz, wm, ws, wn = plain_cohort(top[p].numpy(), k, skip, cohort, floor)
        where = (p, k, skip, cohort)
        assert _ubits(z)[p].tolist() == wz, where
        assert int(_ubits(mu)[p]) == wm and int(_ubits(sigma)[p]) == ws and int(n[p]) == wn, where


def ranked_rows(P, K, seed, nan_from=None):
    """Rows as ``rank_select`` returns them: descending, with ties, NaN from column ``nan_from`` on."""
    gen = torch.Generator().manual_seed(seed)
    t = (torch.randn(P, K, generator=gen) * 4).round() / 4 + torch.rand(P, 1, generator=gen)
    t = t.sort(dim=1, descending=True).values
    if nan_from is not None:
        t[:, nan_from:] = NAN
    return t.contiguous()


# ------------------------------------------------------------------------------- group_topr: the statement
@pytest.mark.parametrize("name", sorted(all_cases()))
def test_topr_against_the_plain_definition(name):
    s, groups = cases()[name]
    off, pos = _csr(groups)
    got = {r: ops.group_topr(s, off, pos, r) for r in RS}
    _, mb = ops.group_scores(s, off, pos, "max")
    worst = 0.0
    for r in RS:
        assert got[r][0].dtype == torch.float32 and got[r][1].dtype == torch.int32
        assert tuple(got[r][0].shape) == (s.shape[0], len(groups)) and torch.equal(got[r][1], mb), (name, r)
    for p in range(s.shape[0]):
        row = s[p].numpy()
        for g, members in enumerate(groups):
            order = _order(row, members) if members else None
            for r in RS:
                wb, wbest = plain_topr(row, members, r, order)
                assert int(_ubits(got[r][0])[p, g]) == wb and int(got[r][1][p, g]) == wbest, (name, p, g, r)
                x = row[order[:min(r, len(members))]].astype(np.float64) if members else np.zeros(0)
                if members and np.isfinite(x).all():
                    rp = len(x)
                    err, bound = abs(float(got[r][0][p, g]) - x.mean()), rp * 2.0 ** -23 * np.abs(x).max()
                    assert err <= bound, (name, p, g, r, err, bound)
                    worst = max(worst, err / bound if bound else 0.0)
    print("MEASURE top-r %s: worst error over bound %.3g" % (name, worst))


def test_topr_per_row_structures():
    s, off, pos, shared, other = per_row_case()
    for r in RS:
        val, gb = ops.group_topr(s, off, pos, r)
        assert torch.equal(gb, ops.group_scores(s, off, pos, "max")[1])
        for p, groups in enumerate((shared, other, shared)):
            row = s[p].numpy()
            for g, members in enumerate(groups):
                wb, wbest = plain_topr(row, members, r)
                assert int(_ubits(val)[p, g]) == wb and int(gb[p, g]) == wbest, (r, p, g)


def test_topr_one_is_the_max_as_a_number():
    """r = 1: s = +0.0 + x1, over 1.  The value is the max fuse's; the bits differ only where the best entry is
    -0.0 (0.0 + -0.0 is +0.0) or a NaN (written as 0x7FC00000 whatever its bits were)."""
    for name, (s, groups) in cases().items():
        off, pos = _csr(groups)
        one, _ = ops.group_topr(s, off, pos, 1)
        mx, _ = ops.group_scores(s, off, pos, "max")
        assert bool(((one == mx) | (torch.isnan(one) & torch.isnan(mx))).all()), name
        differ = _bits(one) != _bits(mx)
        assert bool((~differ | torch.isnan(mx) | (_bits(mx) == -(1 << 31))).all()), name
    row = torch.tensor([[-0.0, -1.0, NAN, NAN]])
    off, pos = _csr([[0, 1], [2, 3], [0]])
    one, gb = ops.group_topr(row, off, pos, 1)
    assert _bits(one)[0].tolist() == [0, QNAN, 0] and gb[0].tolist() == [0, 2, 0]


def test_topr_special_values():
    row = torch.tensor([[1.0, NAN, INF, -INF, 3.0, 3.0, 0.5, -0.0, 0.0, 2.0]])
    groups = [[0, 1], [1, 0, 9], [2, 0], [2, 3], [4, 5, 6], [7, 8], [], [1], [3, 0, 9], [6, 6, 6]]
    off, pos = _csr(groups)
    want = {1: [1.0, 2.0, INF, INF, 3.0, 0.0, None, None, 2.0, 0.5],
            2: [None, 1.5, INF, None, 3.0, 0.0, None, None, 1.5, 0.5],
            3: [None, None, INF, None, 6.5 / 3, 0.0, None, None, -INF, 0.5]}
    for r, ws in want.items():
        val, gb = ops.group_topr(row, off, pos, r)
        assert gb[0].tolist() == [0, 9, 2, 2, 4, 8, -1, 1, 9, 6], r
        for g, w in enumerate(ws):
            if w is None:
                assert _bits(val)[0, g].item() == QNAN, (r, g)                  # NaN entered: fewer numbers than r'
            else:
                assert val[0, g].item() == pytest.approx(w, rel=1e-6), (r, g)
            assert int(_ubits(val)[0, g]) == plain_topr(row[0].numpy(), groups[g], r)[0], (r, g)
        assert _bits(val)[0, 5].item() == 0                                      # zeros: the sum starts at +0.0


def test_topr_composition_independence():
    s, groups = cases()["counts-P3"]
    off, pos = _csr(groups)
    for r in (2, 16):
        full, fb = ops.group_topr(s, off, pos, r)
        for g in (0, 3, 5, 8, 10):
            alone, ab = ops.group_topr(s[1:2], *_csr([groups[g]]), r)
            assert torch.equal(_bits(alone[0]), _bits(full[1, g:g + 1])) and int(ab[0, 0]) == int(fb[1, g]), (r, g)
            # other neighbours, another P and S
            mixed, mb = ops.group_topr(s[:2], *_csr([groups[2], [], groups[g], groups[0]]), r)
            assert torch.equal(_bits(mixed[:, 2]), _bits(full[:2, g])) and torch.equal(mb[:, 2], fb[:2, g]), (r, g)


# ---------------------------------------------------------------------------- cohort_decide: the statement
@pytest.mark.parametrize("K,skip,cohort", [(1, 1, 32), (2, 0, 2), (40, 1, 32), (64, 0, 64), (65, 1, 64), (130, 5, 31),
                                           (300, 0, 300), (1024, 5, 1019), (1100, 1, 1023)])
def test_cohort_against_the_plain_definition(K, skip, cohort):
    top = ranked_rows(3, K, 100 + K, nan_from=None)
    top[1, max(1, K * 2 // 3):] = NAN                        # row 1: a NaN tail beginning inside the window
    for k in sorted({1, min(K, 5), min(K, 70)}):
        check_cohort(top, k, skip, cohort)


DISTRIBUTIONS = {
    "normal": lambda n, gen: torch.randn(n, generator=gen),
    "uniform": lambda n, gen: torch.rand(n, generator=gen),
    "offset-logit": lambda n, gen: 12.0 + torch.randn(n, generator=gen),
    "sigmoid": lambda n, gen: torch.sigmoid(2.0 * torch.randn(n, generator=gen)),
}


@pytest.mark.parametrize("dist", sorted(DISTRIBUTIONS))
def test_cohort_against_float64(dist):
    gen = torch.Generator().manual_seed(21)
    worst, held = 0.0, 0
    for n in (2, 3, 17, 63, 64, 65, 200, 511, 1023):
        rows = torch.stack([DISTRIBUTIONS[dist](n + 1, gen) for _ in range(6)]).sort(dim=1, descending=True).values
        _, mu, sigma, cn, _ = ops.cohort_decide(rows.contiguous(), 1, 1, n)
        assert cn.tolist() == [n] * 6
        x = rows[:, 1:].double()
        mu64, sg64, top = x.mean(1), x.std(1, unbiased=False), x.abs().max(1).values
        for p in range(6):
            if float(sg64[p]) < 0.05 * float(top[p]):
                continue
            bound = n * 2.0 ** -23 * float(top[p])
            e_mu, e_sg = abs(float(mu[p]) - float(mu64[p])), abs(float(sigma[p]) - float(sg64[p]))
            assert e_mu <= bound and e_sg <= bound, (dist, n, p, e_mu, e_sg, bound)
            worst, held = max(worst, e_mu / bound, e_sg / bound), held + 1
    assert held >= 27, (dist, held)                             # the condition on sigma leaves most rows in
    print("MEASURE cohort %s: worst error over bound %.3g on %d rows" % (dist, worst, held))


def edge_rows():
    """(top (P, 8), what each row is) for k = 3, skip = 1, cohort = 4: the window is columns 1 .. 4."""
    rows = [
        ([9.0, 5.0, 4.0, 3.0, 2.0, 1.0, 0.5, 0.25], "plain"),
        ([9.0, 5.0, NAN, NAN, NAN, NAN, NAN, NAN], "n = 1"),
        ([9.0, 5.0, 4.0, NAN, NAN, NAN, NAN, NAN], "a NaN tail beginning inside the window, n = 2"),
        ([NAN] * 8, "all NaN, n = 0"),
        ([INF, 5.0, 4.0, 3.0, 2.0, 1.0, 0.5, 0.25], "+inf at rank 1"),
        ([INF, INF, 4.0, 3.0, 2.0, 1.0, 0.5, 0.25], "+inf inside the cohort"),
        ([9.0, 2.0, 2.0, 2.0, 2.0, 1.0, 0.5, 0.25], "a constant cohort"),
        ([2.0, 2.0, 2.0, 0.0, -0.0, -0.0, -1.0, -1.0], "ties and -0.0"),
        ([0.0, -0.0, -0.0, -0.0, -0.0, -1.0, -2.0, -INF], "a cohort of -0.0"),
        ([5.0, 4.0, 3.0, 2.0, -INF, -INF, NAN, NAN], "-inf inside the cohort"),
    ]
    return torch.tensor([r for r, _ in rows]), [w for _, w in rows]


def test_cohort_edge_rows():
    top, what = edge_rows()
    check_cohort(top, 3, 1, 4)
    z, mu, sigma, n, acc = ops.cohort_decide(top, 3, 1, 4, threshold=3.0)
    at = what.index
    assert n.tolist() == [4, 1, 2, 0, 4, 4, 4, 4, 4, 4]
    for name in ("n = 1", "all NaN, n = 0"):
        p = at(name)
        assert _bits(mu)[p].item() == QNAN and _bits(sigma)[p].item() == QNAN and _bits(z)[p].tolist() == [QNAN] * 3
        assert acc[p].tolist() == [0, 0, 0]
    p = at("+inf at rank 1")
    assert float(z[p, 0]) == INF and acc[p].tolist() == [1, 0, 0] and math.isfinite(float(sigma[p]))
    p = at("+inf inside the cohort")
    assert _bits(z)[p].tolist() == [QNAN] * 3 and acc[p].tolist() == [0, 0, 0] and float(mu[p]) == INF
    assert _bits(sigma)[p].item() == QNAN
    p = at("a constant cohort")                              # sigma = 0: the floor divides
    assert float(sigma[p]) == 0.0 and float(mu[p]) == 2.0
    assert z[p].tolist() == [float(F(7.0) / F(1e-6)), 0.0, 0.0] and acc[p].tolist() == [1, 0, 0]
    assert float(ops.cohort_decide(top, 3, 1, 4, sigma_floor=0.5)[0][p, 0]) == 14.0
    p = at("a cohort of -0.0")
    assert _bits(mu)[p].item() == 0 and _bits(sigma)[p].item() == 0          # the lanes start at +0.0
    assert _ubits(z)[p].tolist() == [0, 0x80000000, 0x80000000]              # (-0.0 - +0.0) / s
    p = at("-inf inside the cohort")
    assert float(mu[p]) == -INF and _bits(sigma)[p].item() == QNAN and acc[p].tolist() == [0, 0, 0]
    # the window past the row's end: K = 1, and skip >= K
    for K, skip in ((1, 1), (3, 3), (3, 7)):
        z, mu, sigma, n, acc = ops.cohort_decide(top[:, :K].contiguous(), 1, skip, 4, threshold=-INF)
        assert n.tolist() == [0] * 10 and _bits(z).view(-1).tolist() == [QNAN] * 10 and acc.view(-1).tolist() == [0] * 10
    # thresholds at the infinities: every non-NaN z accepted, none accepted
    z, _, _, _, acc = ops.cohort_decide(top, 3, 1, 4, threshold=-INF)
    assert torch.equal(acc, (~torch.isnan(z)).to(torch.int32))
    acc = ops.cohort_decide(top, 3, 1, 4, threshold=INF)[4]
    p = at("+inf at rank 1")                                 # accept is z >= threshold: z = +inf reaches +inf
    assert acc[p].tolist() == [1, 0, 0] and not bool(acc[torch.arange(10) != p].any())
    # normalize=False: the raw score against the threshold, no statistics
    z, mu, sigma, n, acc = ops.cohort_decide(top, 3, threshold=4.0, normalize=False)
    assert z is None and mu is None and sigma is None and n is None and acc.dtype == torch.int32
    assert torch.equal(acc, (top[:, :3] >= 4.0).to(torch.int32)) and acc[at("all NaN, n = 0")].tolist() == [0, 0, 0]
    z, _, _, _, acc = ops.cohort_decide(top, 3, 1, 4)
    assert acc is None and z is not None


# ---------------------------------------------------------------------------------------- refusals
def test_refusals(monkeypatch):
    def trap(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", trap)
    s = torch.zeros(2, 10)
    off, pos = _csr([[0, 1], [5]])
    ops.group_topr(s, off, pos, 2)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    for kw, msg in ((dict(r=0), r"r = 0 outside \[1, 16\]"), (dict(r=17), r"r = 17 outside \[1, 16\]"),
                    (dict(r=2.0), "an integer"), (dict(r=True), "an integer"),
                    (dict(off=i32([1, 2, 3])), "group_topr: offsets must start at 0"),
                    (dict(off=i32([0, 3, 2])), "must not fall"), (dict(off=i32([0, 2, 4])), "pos holds 3"),
                    (dict(pos=i32([0, 10, 5])), r"outside \[0, 10\)"), (dict(pos=i32([0, -1, 5])), r"outside \[0, 10\)"),
                    (dict(off=off.long()), "group_topr: off must be a int32"), (dict(pos=pos.long()), "pos must be a int32"),
                    (dict(scores=s.double()), "group_topr: scores must be a .* fp32"),
                    (dict(scores=torch.zeros(65536, 1), pos=i32([0, 0, 0])), "65535 rows"),
                    (dict(off=torch.stack([off, off]), pos=pos), "shared structure"),
                    (dict(off=torch.stack([off] * 3), pos=torch.stack([pos] * 3)), "per-row structures"),
                    (dict(off_host=i32([0, 1, 3, 3])), "host copies"),
                    (dict(gscore=torch.zeros(2, 3)), "group_topr gscore"),
                    (dict(gbest=torch.zeros(2, 2)), "gbest contiguous int32")):
        a = dict(scores=s, off=off, pos=pos, r=2)
        a.update(kw)
        with pytest.raises(_lib.FpmError, match=msg):
            ops.group_topr(a.pop("scores"), a.pop("off"), a.pop("pos"), a.pop("r"), **a)

    top = ranked_rows(2, 40, 3)
    ops.cohort_decide(top, 3)
    for kw, msg in ((dict(top=top.double()), "fp32"), (dict(top=top[0]), r"\(P, K\) fp32"),
                    (dict(top=top[:, ::2]), "contiguous"), (dict(k=0), r"k = 0 outside \[1, K = 40\]"),
                    (dict(k=41), r"k = 41 outside"), (dict(k=2.0), "k must be an integer"),
                    (dict(cohort=1), "cohort = 1"), (dict(skip=-1), "skip = -1"),
                    (dict(skip=2, cohort=1023), r"skip \+ cohort <= 1024"), (dict(cohort=32.0), "cohort must be an integer"),
                    (dict(threshold=NAN), "threshold is NaN"), (dict(sigma_floor=0.0), "sigma_floor"),
                    (dict(sigma_floor=-1.0), "sigma_floor"), (dict(sigma_floor=INF), "sigma_floor"),
                    (dict(sigma_floor=NAN), "sigma_floor"), (dict(sigma_floor=1e-50), "sigma_floor"),
                    (dict(normalize=False), "nothing to compute"),
                    (dict(top=torch.zeros(65536, 1), k=1), "65535 rows")):
        a = dict(top=top, k=3)
        a.update(kw)
        with pytest.raises(_lib.FpmError, match=msg):
            ops.cohort_decide(a.pop("top"), a.pop("k"), **a)
    ops.cohort_decide(top, 3, skip=1, cohort=1023)             # skip + cohort = 1024 is the largest window

    net = types.SimpleNamespace(training=False, use_graphs=False, dtype_mode="f32")   # refused before the net is asked
    lab = hand_index("f32")
    lab.set_subjects([0, 0, 1])
    probe = {"n": 3}
    ok = dict(by="subject", fuse="mean")
    for call in (lambda **kw: gallery.identify(net, probe, lab, **kw), lambda **kw: gallery.identify_many(net, lab, lab, **kw)):
        for kw, msg in ((dict(top_r=2), "top_r without by='subject'"), (dict(top_r=2, fuse="mean"), "top_r without by"),
                        (dict(by="subject", top_r=2), "top_r needs fuse='mean'"),
                        (dict(by="subject", fuse="max", top_r=2), "top_r needs fuse='mean'"),
                        (dict(top_r=0, **ok), r"top_r = 0 outside \[1, 16\]"), (dict(top_r=17, **ok), "top_r = 17 outside"),
                        (dict(top_r=2.0, **ok), "an integer"), (dict(normalize="z"), "normalize must be one of"),
                        (dict(normalize="cohort", cohort=1), "cohort = 1"),
                        (dict(normalize="cohort", cohort=1024, cohort_skip=1), r"cohort_skip \+ cohort <= 1024"),
                        (dict(normalize="cohort", cohort_skip=-1), "cohort_skip = -1"),
                        (dict(threshold=NAN), "threshold is NaN"), (dict(normalize="cohort", threshold=NAN), "threshold is NaN"),
                        (dict(normalize="cohort", sigma_floor=0.0), "sigma_floor")):
            with pytest.raises(_lib.FpmError, match=msg):
                call(**kw)


# ------------------------------------------------------------------------------ the stage on CPU tensors
def _check_stage(keys, ranked, rank, k, opt, by_subject):
    """The stage's keys against ``rank_select`` plus the plain definitions on the same ranked rows."""
    Q, X = ranked.shape
    K = min(X, max(k, opt["skip"] + opt["cohort"]))
    _, top = ops.rank_select(ranked, K)
    assert torch.equal(_bits(top[:, :k]), _bits(rank["top_score"]))           # the first k columns are top_score
    want = set()
    if opt["normalize"]:
        want |= {"top_z", "cohort_mu", "cohort_sigma", "cohort_n"}
        check_cohort(top, k, opt["skip"], opt["cohort"], opt["sigma_floor"],
                     got=(keys["top_z"], keys["cohort_mu"], keys["cohort_sigma"], keys["cohort_n"], None))
        assert keys["cohort_n"].dtype == torch.int32 and tuple(keys["cohort_mu"].shape) == (Q,)
    if opt["threshold"] is not None:
        want |= {"accept", "match"}
        v = keys["top_z"] if opt["normalize"] else rank["top_score"]
        assert keys["accept"].dtype == torch.bool and torch.equal(keys["accept"], v >= opt["threshold"])
        first = rank["top_subject" if by_subject else "top_idx"][:, 0].long()
        assert keys["match"].dtype == torch.int64
        assert keys["match"].tolist() == [int(f) if a else -1 for f, a in zip(first, keys["accept"][:, 0])]
    assert set(keys) == want


def _opts(**kw):
    a = dict(top_r=None, normalize=None, cohort=32, cohort_skip=1, sigma_floor=1e-6, threshold=None)
    a.update(kw)
    return gallery._check_open("identify", a["top_r"] is not None, "mean", a["top_r"], a["normalize"], a["cohort"],
                               a["cohort_skip"], a["sigma_floor"], a["threshold"])


STAGE_OPTS = [dict(normalize="cohort"), dict(normalize="cohort", threshold=1.5), dict(threshold=0.25),
              dict(normalize="cohort", cohort=5, cohort_skip=2, threshold=-INF),
              dict(normalize="cohort", cohort=3, cohort_skip=0, sigma_floor=0.5, threshold=INF)]


@pytest.mark.parametrize("kw", STAGE_OPTS)
def test_stage_entry_level(kw, monkeypatch):
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("the library was called"))
    gen = torch.Generator().manual_seed(31)
    sc = (torch.randn(4, 50, generator=gen) * 3).round() / 3             # ties
    sc[2, 7] = NAN
    ents = torch.randperm(50, generator=gen).to(torch.int32)
    opt = _opts(**kw)
    assert opt["stage"] and opt["top_r"] is None
    for topk in (1, 4, 60):
        rank = gallery._entry_ranking(sc, ents, topk)
        keys = gallery._open_set(sc, rank, opt)
        _check_stage(keys, sc, rank, min(topk, 50), opt, False)
    # a short list: fewer candidates than the cohort asks for (K = X)
    rank = gallery._entry_ranking(sc[:, :3].contiguous(), ents[:3], 2)
    _check_stage(gallery._open_set(sc[:, :3].contiguous(), rank, opt), sc[:, :3].contiguous(), rank, 2, opt, False)


@pytest.mark.parametrize("top_r", [None, 1, 2, 3])
def test_stage_subject_level_ragged(top_r, monkeypatch):
    """Ragged per-probe pair lists, as the probe-set exact stage hands them to ``_subject_ranking``: probe 1's
    third subject is emptied (leave-one-out took its only entry), so its fused score is NaN: it ranks last and is
    outside the cohort."""
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("the library was called"))
    gen = torch.Generator().manual_seed(32)
    counts = [[3, 1, 2, 4, 1, 3, 2], [2, 2, 0, 4, 1, 1, 3], [1, 1, 1, 1, 1, 1, 1]]
    rows = [torch.randn(sum(c), generator=gen) for c in counts]
    ents = [torch.randperm(100, generator=gen)[:sum(c)] for c in counts]
    offs = [torch.tensor([0] + list(np.cumsum(c))) for c in counts]
    labels = torch.stack([torch.randperm(40, generator=gen)[:7] for _ in counts])
    opt = _opts(top_r=top_r, normalize="cohort", cohort=4, cohort_skip=1, threshold=1.0)
    assert opt["top_r"] == top_r
    rank = gallery._subject_ranking(rows, ents, offs, labels, "mean", 7, torch.device("cpu"), top_r)
    gsc = rank["subject_score"]
    for q, c in enumerate(counts):                           # the fuse is the op's statement on each probe's row
        off32 = offs[q].to(torch.int32)
        pos32 = torch.arange(sum(c), dtype=torch.int32)
        want = ops.group_scores(rows[q].view(1, -1), off32, pos32, "mean") if top_r is None else \
            ops.group_topr(rows[q].view(1, -1), off32, pos32, top_r)
        assert torch.equal(_bits(gsc[q]), _bits(want[0][0]))
    assert bool(torch.isnan(gsc[1, 2])) and int(rank["top_subject"][1, 6]) == int(labels[1, 2])
    keys = gallery._open_set(gsc, rank, opt)
    _check_stage(keys, gsc, rank, 7, opt, True)
    assert keys["cohort_n"].tolist() == [4, 4, 4] and _bits(keys["top_z"])[1, 6].item() == QNAN
    assert not bool(keys["accept"][1, 6])
    # a cohort that reaches the emptied subject leaves it out: 7 subjects, skip 1, cohort 6 -> n = 5 for probe 1
    wide = gallery._open_set(gsc, rank, _opts(normalize="cohort", cohort=6))
    assert wide["cohort_n"].tolist() == [6, 5, 6]


def test_keywords_off_is_off():
    opt = _opts()
    assert not opt["stage"] and opt["top_r"] is None

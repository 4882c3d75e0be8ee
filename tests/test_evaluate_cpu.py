"""Search evaluation on the host: the statements of ``ops.mate_rank`` / ``score_census`` / ``score_select`` (the
CPU paths the kernels are held to) against brute force, ``evaluate.far_threshold``'s defining property,
``evaluate.verification_report`` against scikit-learn's recorded outputs, and the funnel arithmetic of
``evaluate.funnel`` on hand-made result dicts.
"""
import os

import numpy as np
import pytest
import torch

from fpm import _lib, evaluate, ops

QNAN = 0x7FC00000
SPECIALS = (0.0, -0.0, float("inf"), float("-inf"), float("nan"))


def _bits(t):
    return t.contiguous().view(torch.int32)


def eval_case(P, G, seed, per_row=False, specials=True):
    """Scores from {-1, 0, 1} (ties) with +-0, +-inf and NaN sprinkled in; labels from a few subjects with some
    columns labelled -1; an ``own`` column for every other row."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(-1, 2, (P, G), generator=g).to(torch.float32)
    if specials:
        for v in SPECIALS:
            at = torch.rand(P, G, generator=g) < 0.08
            s = torch.where(at, torch.tensor(v), s)
    nlab = max(2, min(5, G))
    col = torch.randint(-1, nlab, (P, G) if per_row else (G,), generator=g).to(torch.int32)
    row = torch.randint(0, nlab, (P,), generator=g).to(torch.int32)
    own = torch.randint(0, G, (P,), generator=g).to(torch.int32)
    own[::2] = -1
    return s, row, col, own


def key_above(sa, ja, sb, jb):
    """``rank_key`` order, spelled out: does (score sa, column ja) rank above (sb, jb)?"""
    def order(x):
        b = int(np.float32(x).view(np.uint32))
        if (b & 0x7FFFFFFF) > 0x7F800000:
            return 0
        return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)
    a, b = order(sa), order(sb)
    return a > b or (a == b and ja < jb)


def brute_mate_rank(s, row, col, own):
    P, G = s.shape
    cols, scs, ranks = [], [], []
    for p in range(P):
        cl = col[p] if col.dim() == 2 else col
        gen = [j for j in range(G) if cl[j] >= 0 and j != int(own[p]) and cl[j] == row[p]]
        imp = [j for j in range(G) if cl[j] >= 0 and j != int(own[p]) and cl[j] != row[p]]
        if not gen:
            cols.append(-1), scs.append(QNAN), ranks.append(-1)
            continue
        m = gen[0]
        for j in gen[1:]:
            if key_above(float(s[p, j]), j, float(s[p, m]), m):
                m = j
        cols.append(m)
        scs.append(int(_bits(s[p, m:m + 1])[0]))
        ranks.append(sum(key_above(float(s[p, j]), j, float(s[p, m]), m) for j in imp))
    return cols, scs, ranks


@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("G", [1, 2, 65])
@pytest.mark.parametrize("P", [1, 3])
def test_mate_rank_against_brute_force(P, G, per_row):
    for seed in range(4):
        s, row, col, own = eval_case(P, G, 100 * G + 10 * P + seed, per_row)
        if seed == 1:
            row[0] = 77                                           # a row without a mate
        if seed == 2:                                             # a row whose only mate is its own column
            cl = col[0] if per_row else col
            cl[:] = torch.where(cl == row[0], torch.tensor(-1, dtype=torch.int32), cl)
            cl[G - 1] = row[0]
            own[0] = G - 1
        mc, ms, mr = ops.mate_rank(s, row, col, own)
        assert mc.dtype == torch.int32 and ms.dtype == torch.float32 and mr.dtype == torch.int32
        cols, scs, ranks = brute_mate_rank(s, row, col, own)
        assert mc.tolist() == cols and _bits(ms).tolist() == scs and mr.tolist() == ranks, (P, G, per_row, seed)
        if seed in (1, 2):
            assert (int(mc[0]), int(_bits(ms)[0]), int(mr[0])) == (-1, QNAN, -1)
        # own=None is own = -1 everywhere
        none = torch.full_like(own, -1)
        for a, b in zip(ops.mate_rank(s, row, col), ops.mate_rank(s, row, col, none)):
            assert torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b)


def test_mate_rank_orders_zeros_and_nan():
    s = torch.tensor([[0.0, -0.0, float("nan"), 0.0, float("nan")]])
    col = torch.tensor([1, 0, 0, 0, 0], dtype=torch.int32)
    row = torch.tensor([0], dtype=torch.int32)
    # mate: +0 at column 3 (above -0 and both NaN); the impostor +0 at column 0 ties and has the lower column
    assert [int(t[0]) for t in ops.mate_rank(s, row, col)[::2]] == [3, 1]
    # without column 3 the mate is -0 at column 1, still below the impostor's +0
    col = torch.tensor([1, 0, 0, -1, 0], dtype=torch.int32)
    assert [int(t[0]) for t in ops.mate_rank(s, row, col)[::2]] == [1, 1]
    col = torch.tensor([1, 1, 1, 1, 0], dtype=torch.int32)       # the mate is a NaN: after the other NaN (lower column)
    mc, ms, mr = ops.mate_rank(s, row, col)
    assert int(mc[0]) == 4 and bool(torch.isnan(ms[0])) and int(mr[0]) == 4


@pytest.mark.parametrize("P,G,T", [(1, 1, 1), (3, 65, 2), (3, 65, 7), (5, 300, 4095)])
def test_census_totals_and_bins(P, G, T):
    s, row, col, own = eval_case(P, G, 7 * G + T)
    edges = torch.linspace(-1.0, 1.0, T) if T > 1 else torch.tensor([0.0])
    gen, imp, skipped = ops.score_census(s, row, col, edges, own)
    assert gen.dtype == torch.int64 and tuple(gen.shape) == (T + 1,) and tuple(imp.shape) == (T + 1,)
    assert tuple(skipped.shape) == (3,)
    assert int(gen.sum() + imp.sum() + skipped.sum()) == P * G
    # brute force
    want = np.zeros((2, T + 1), dtype=np.int64)
    sk = [0, 0, 0]
    e = edges.tolist()
    for p in range(P):
        for j in range(G):
            x = float(s[p, j])
            if col[j] < 0 or j == int(own[p]):
                sk[2] += 1
                continue
            c = 0 if col[j] == row[p] else 1
            if x != x:
                sk[c] += 1
            else:
                want[c, sum(1 for v in e if v <= x)] += 1
    assert gen.tolist() == want[0].tolist() and imp.tolist() == want[1].tolist() and skipped.tolist() == sk


def test_census_edge_goes_up_and_infinities():
    edges = torch.tensor([-0.5, 0.0, 0.5])
    s = torch.tensor([[-0.5, 0.0, 0.5, float("-inf"), float("inf"), -0.0, 0.49999997]])
    row = torch.tensor([0], dtype=torch.int32)
    col = torch.zeros(7, dtype=torch.int32)
    gen, imp, skipped = ops.score_census(s, row, col, edges)
    # -0.5 -> bin 1, 0.0 and -0.0 -> bin 2, 0.5 and +inf -> bin 3, -inf -> bin 0, just under 0.5 -> bin 2
    assert gen.tolist() == [1, 1, 3, 2] and int(imp.sum()) == 0 and skipped.tolist() == [0, 0, 0]


@pytest.mark.parametrize("cls", ops.SCORE_CLASSES)
def test_score_select_against_sort(cls):
    s, row, col, own = eval_case(4, 130, 5)
    gen, imp = ops.score_classes(s, row, col, own)
    vals = s[(gen if cls == "genuine" else imp) & ~torch.isnan(s)]
    order = sorted(vals.tolist(), key=lambda x: (x, np.signbit(x) == 0), reverse=True)   # -0 below +0
    n = len(order)
    assert n > 20
    for k in [1, 2, n // 3, n // 2, n - 1, n]:                    # scores from {-1, 0, 1}: ties straddle every k
        v, count = ops.score_select(s, row, col, cls, k, own)
        assert count == n and v.dtype == torch.float32 and v.dim() == 0
        assert int(_bits(v.view(1))[0]) == int(_bits(torch.tensor([order[k - 1]]))[0]), (cls, k)
    v, count = ops.score_select(s, row, col, cls, n + 1, own)
    assert count == n and int(_bits(v.view(1))[0]) == QNAN


def test_refusals_host():
    s, row, col, own = eval_case(3, 9, 1)
    edges = torch.tensor([0.0, 1.0])
    bad = [
        (lambda: ops.mate_rank(s.double(), row, col), "fp32"),
        (lambda: ops.mate_rank(s, row.long(), col), "int32"),
        (lambda: ops.mate_rank(s, row, col[:5]), "col_lab of shape"),
        (lambda: ops.mate_rank(s, row[:2], col), "row_lab"),
        (lambda: ops.mate_rank(s, row, col, own.long()), "int32"),
        (lambda: ops.score_census(s, row, col, torch.tensor([1.0, 0.0])), "ascending"),
        (lambda: ops.score_census(s, row, col, torch.tensor([0.0, 0.0])), "ascending"),
        (lambda: ops.score_census(s, row, col, torch.tensor([0.0, float("inf")])), "finite"),
        (lambda: ops.score_census(s, row, col, torch.tensor([float("nan")])), "finite"),
        (lambda: ops.score_census(s, row, col, torch.zeros(0)), "outside"),
        (lambda: ops.score_census(s, row, col, torch.arange(4096.0)), "outside"),
        (lambda: ops.score_census(s, row, col, edges.double()), "fp32"),
        (lambda: ops.score_select(s, row, col, "impostor", 0), "k = 0"),
        (lambda: ops.score_select(s, row, col, "impostor", 1.0), "integer"),
        (lambda: ops.score_select(s, row, col, "mate", 1), "cls"),
    ]
    for call, msg in bad:
        with pytest.raises(_lib.FpmError, match=msg):
            call()


# ------------------------------------------------------------------------------------- far_threshold
@pytest.mark.parametrize("far", [0.0, 1e-3, 0.5, 1.0])
def test_far_threshold_property(far):
    """count(imp >= t) <= k < count(imp >= prev_float(t)) on 2000 impostors, 40 % of them tied."""
    g = torch.Generator().manual_seed(11)
    imp = torch.randn(2000, generator=g)
    tied = torch.rand(2000, generator=g) < 0.4
    imp = torch.where(tied, torch.round(imp * 2) / 2, imp)       # the tied ones share a few values
    gen = torch.randn(100, generator=g) + 2.0
    s = torch.cat([imp, gen]).view(4, 525)
    col = torch.cat([torch.zeros(2000), torch.ones(100)]).to(torch.int32).view(4, 525)
    row = torch.ones(4, dtype=torch.int32)
    r = evaluate.far_threshold(s, row, col, far)
    k = int(np.floor(np.float64(far) * 2000))
    assert r["k"] == k and r["impostors"] == 2000 and r["genuines"] == 100
    t = np.float32(r["threshold"])
    impn = imp.numpy()
    assert float(t) == r["threshold"]
    if k >= 2000:
        assert t == -np.inf and r["false_accepts"] == 2000 and r["far"] == 1.0 and r["frr"] == 0.0
        return
    below = np.nextafter(t, np.float32(-np.inf))
    assert int((impn >= t).sum()) <= k < int((impn >= below).sum())
    assert r["false_accepts"] == int((impn >= t).sum()) and r["far"] == r["false_accepts"] / 2000
    assert r["false_rejects"] == int((gen.numpy() < t).sum()) and r["frr"] == r["false_rejects"] / 100


def test_score_report():
    g = torch.Generator().manual_seed(3)
    s = torch.cat([torch.randn(3, 400, generator=g), torch.randn(3, 40, generator=g) + 3.0], 1).contiguous()
    s[0, 5], s[1, 410] = float("nan"), float("inf")
    col = torch.cat([torch.zeros(400), torch.ones(40)]).to(torch.int32)
    row = torch.ones(3, dtype=torch.int32)
    rep = evaluate.score_report(s, row, col, far=(1e-2, 0.1))
    T = int(rep["edges"].numel())
    assert T == 1023 and float(rep["edges"][0]) == float(s[torch.isfinite(s)].min())
    assert int(rep["gen"].sum() + rep["imp"].sum() + rep["skipped"].sum()) == s.numel()
    assert rep["skipped"].tolist() == [0, 1, 0]
    e = rep["edges"].numpy()
    impv, genv = s[:, :400].numpy().ravel(), s[:, 400:].numpy().ravel()
    impv = impv[~np.isnan(impv)]
    far = np.array([(impv >= t).sum() for t in e]) / impv.size
    frr = np.array([(genv < t).sum() for t in e]) / genv.size
    assert np.array_equal(rep["far"], far) and np.array_equal(rep["frr"], frr)
    at = int(np.nanargmin(np.abs(far - frr)))
    assert rep["eer"]["index"] == at and rep["eer"]["threshold"] == float(e[at])
    assert [t["far_target"] for t in rep["thresholds"]] == [1e-2, 0.1]
    assert rep["thresholds"][0]["false_accepts"] <= int(0.01 * impv.size)


# ------------------------------------------------------------------------------ verification_report
def test_verification_report_against_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "verification_metrics.npz"))
    prob, label = z["prob"], z["label"]
    assert prob.size == 300 and np.unique(prob).size < 150       # ties
    r = evaluate.verification_report(prob, label)
    assert [r["tn"], r["fp"], r["fn"], r["tp"]] == z["counts"].tolist()
    assert r["eer_threshold"] == float(z["eer_threshold"])
    assert np.array_equal(r["thresholds"], z["thresholds"])
    for k in ("fpr", "tpr"):
        assert r[k].shape == z[k].shape and float(np.abs(r[k] - z[k]).max()) <= 1e-12, k
    for k in ("accuracy", "precision", "recall", "f1", "roc_auc", "pr_auc", "far", "frr"):
        assert abs(r[k] - float(z[k])) <= 1e-12, (k, r[k], float(z[k]))
    # torch tensors are taken too
    r2 = evaluate.verification_report(torch.from_numpy(prob), torch.from_numpy(label))
    assert r2["roc_auc"] == r["roc_auc"] and r2["tp"] == r["tp"]
    with pytest.raises(_lib.FpmError, match="both present"):
        evaluate.verification_report(prob, np.ones_like(label))


# ------------------------------------------------------------------------------------------- funnel
def _entry_result(pre, short, scores, match=None):
    r = dict(pre_idx=torch.tensor(pre, dtype=torch.int32), short_idx=torch.tensor(short, dtype=torch.int32),
             cls_prob=torch.tensor(scores, dtype=torch.float32))
    if match is not None:
        r["match"] = torch.tensor(match, dtype=torch.int64)
    return r


def test_funnel_entry_level():
    subject = torch.tensor([10, 11, 12, 10, 13, 14])             # entries 0 and 3: two impressions of subject 10
    results = [
        _entry_result([0, 1, 2, 3], [3, 1], [0.9, 0.2], 3),      # mate shortlisted, rank 0, matched to entry 3
        _entry_result([1, 2, 4, 5], [1, 2], [0.5, 0.4], 1),      # mate 12 survives both lists, rank 1; match is 11
        _entry_result([0, 1, 4, 5], [0, 1], [0.3, 0.3], -1),     # mate 13 (entry 4) prescreened, not shortlisted
        _entry_result([0, 1, 2, 3], [0, 1], [0.8, 0.1], 0),      # label 99: non-mated, falsely matched
        _entry_result([2, 3, 4, 5], [2, 3], [0.8, 0.1], -1),     # label 98: non-mated, rejected
    ]
    rep = evaluate.funnel(results, [10, 12, 13, 99, 98], subject, torch.arange(6), ks=(1, 2))
    per = rep["probes"]
    assert [d["mated"] for d in per] == [True, True, True, False, False]
    assert [d["in_prescreen"] for d in per] == [True, True, True, False, False]
    assert [d["in_shortlist"] for d in per] == [True, True, False, False, False]
    assert [d["rank"] for d in per] == [0, 1, -1, -1, -1]
    assert rep["mated"] == 3 and rep["non_mated"] == 2
    assert rep["stages"] == dict(prescreen=1.0, shortlist=2 / 3, exact=2 / 3)
    assert rep["cmc"] == {1: 1 / 3, 2: 2 / 3}
    assert rep["fnir"] == 2 / 3 and rep["fpir"] == 1 / 2
    # exclude_self: probe q is entry q; its own entry is no mate and is ignored in the ranking
    results = [dict(cls_prob=torch.tensor([0.1, 0.95, 0.9, 0.3, 0.4])) for _ in range(2)]
    rep = evaluate.funnel(results, subject[[0, 1]], subject, torch.arange(6), own=torch.tensor([0, 1]), ks=(1, 3))
    per = rep["probes"]
    assert [d["mated"] for d in per] == [True, False]            # entry 3 mates entry 0; subject 11 has one entry
    assert per[0]["in_shortlist"] is None and per[0]["in_prescreen"] is None
    assert per[0]["rank"] == 1 and per[1]["rank"] == -1          # candidates 1 .. 5: entry 3 (0.9) behind entry 2 (0.95)
    assert rep["stages"] == dict(prescreen=None, shortlist=None, exact=1.0) and rep["cmc"] == {1: 0.0, 3: 1.0}
    assert "fnir" not in rep


def test_funnel_subject_level():
    subject = torch.tensor([10, 10, 11, 12])
    mk = lambda short, subs, sc, match: dict(short_subject=torch.tensor(short), subjects=torch.tensor(subs),
                                             subject_score=torch.tensor(sc), match=torch.tensor(match))
    results = [mk([10, 11], [10, 11], [0.7, 0.9], 11),           # mate shortlisted, rank 1, wrong match
               mk([11, 12], [11, 12], [0.7, 0.9], -1),           # mate 10 not shortlisted
               mk([10, 12], [10, 12], [float("nan"), 0.2], 12)]  # non-mated (label 50), accepted
    rep = evaluate.funnel(results, [10, 10, 50], subject, torch.arange(4), by="subject", ks=(1, 2))
    per = rep["probes"]
    assert [d["in_shortlist"] for d in per] == [True, False, False]
    assert [d["rank"] for d in per] == [1, -1, -1]
    assert rep["stages"] == dict(prescreen=None, shortlist=0.5, exact=0.5)
    assert rep["cmc"] == {1: 0.0, 2: 0.5} and rep["fnir"] == 1.0 and rep["fpir"] == 1.0

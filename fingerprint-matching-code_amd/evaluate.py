"""Evaluation of the 1:N search: where each stage loses the true mate, the genuine / impostor score
distributions, FAR thresholds, and the reference's binary-classifier metrics.

The device side is ``ops.mate_rank``, ``ops.score_census`` and ``ops.score_select`` (``csrc/evaluate.hip``):
integer-exact, so every figure here is one answer whatever the schedule.  Labels: a *subject* label per probe
and per gallery entry (``GalleryIndex.subject``; the impressions of one finger share a label).  A probe whose
label is absent from the searched entries is non-mated.

  far_threshold        the smallest fp32 threshold that accepts at most floor(far * N) of N impostor scores
  score_report         the census over a grid of edges, cumulative FAR / FRR, the EER point, FAR thresholds
  stage_ranks          the mate's rank per probe at the descriptor, coarse and coarse-subject stages: CMC and
                       recall at every K from one pass over the score matrices
  search_report        ``identify_many`` unchanged, and the funnel read off its result keys
  verification_report  the reference's evaluate_binary_classifier.py:141-159 in float64 numpy (no sklearn)
"""
import numpy as np
import torch

from . import ops
from ._lib import FpmError

STAGE_BYTES = 256 << 20       # the live score matrix of ``stage_ranks`` stays under this


# ------------------------------------------------------------------------------------------ thresholds
def _i32(t, dev):
    return torch.as_tensor(t).to(device=dev, dtype=torch.int32).contiguous()


def far_threshold(scores, row_lab, col_lab, far, own=None):
    """The decision threshold of a false-accept rate.  N = the number of non-NaN impostor scores
    (``ops.score_classes``), k = floor(float64(far) * N), v = the (k + 1)-th largest impostor score
    (``ops.score_select``), t = the next fp32 above v; k >= N gives t = -inf.  So count(impostor >= t) <= k, and t
    is the smallest fp32 with that property.  -> dict: ``threshold`` (a float holding the fp32 value: what
    ``threshold=`` of ``identify`` takes when ``normalize`` is off), ``k``, ``impostors``, ``genuines`` (non-NaN
    counts), ``false_accepts`` and ``false_rejects`` (counts from a one-edge ``ops.score_census`` at t), ``far``
    and ``frr`` (those over the counts; NaN over an empty class), ``far_target``."""
    far = float(far)
    if not 0.0 <= far <= 1.0:
        raise FpmError("far_threshold: far = %r outside [0, 1]" % far)
    _, n_imp = ops.score_select(scores, row_lab, col_lab, "impostor", 1, own)
    _, n_gen = ops.score_select(scores, row_lab, col_lab, "genuine", 1, own)
    k = int(np.floor(np.float64(far) * np.float64(n_imp)))
    if k >= n_imp:
        t = float("-inf")
        fa, fr = n_imp, 0
    else:
        v, _ = ops.score_select(scores, row_lab, col_lab, "impostor", k + 1, own)
        v = np.float32(float(v))
        if not np.isfinite(v) and v > 0:
            raise FpmError("far_threshold: more than k = %d impostor scores are +inf; no fp32 threshold lies above them"
                           % k)
        t = float(np.nextafter(v, np.float32(np.inf))) if np.isfinite(v) else float(np.finfo(np.float32).min)
        if t == float("inf"):
            raise FpmError("far_threshold: the threshold above %r is +inf (not a finite edge)" % float(v))
        edge = torch.tensor([t], dtype=torch.float32, device=scores.device)
        gen, imp, _ = ops.score_census(scores, row_lab, col_lab, edge, own)
        fa, fr = int(imp[1]), int(gen[0])
    return dict(threshold=t, k=k, impostors=n_imp, genuines=n_gen, false_accepts=fa, false_rejects=fr,
                far=fa / n_imp if n_imp else float("nan"), frr=fr / n_gen if n_gen else float("nan"), far_target=far)


def default_edges(scores, count=1023):
    """``count`` evenly spaced fp32 edges between the smallest and the largest finite score (fewer where fp32
    cannot tell neighbours apart; one edge when all finite scores are equal)."""
    fin = scores[torch.isfinite(scores)]
    if fin.numel() == 0:
        raise FpmError("score_report: no finite score to place the default edges by")
    lo, hi = float(fin.min()), float(fin.max())
    e = torch.linspace(lo, hi, int(count), dtype=torch.float64).to(torch.float32)
    return torch.unique(e).to(scores.device).contiguous()


def score_report(scores, row_lab, col_lab, own=None, edges=None, far=(1e-2, 1e-3, 1e-4)):
    """The score distributions of a labelled matrix -> dict:
      edges (T,), gen, imp (T + 1,), skipped (3,)   ``ops.score_census`` (host tensors); ``edges`` None:
                                                    ``default_edges``
      far, frr (T,) float64     at threshold edges[i]: impostors >= it over impostors, genuines < it over genuines
      eer                       dict(index, threshold, far, frr, eer): the first edge that minimises |far - frr|
                                (the rule of the reference's evaluate_binary_classifier.py:143 on the grid),
                                eer = (far + frr) / 2
      thresholds                one ``far_threshold`` per rate of ``far``"""
    if edges is None:
        edges = default_edges(scores)
    gen, imp, skipped = (t.cpu() for t in ops.score_census(scores, row_lab, col_lab, edges, own))
    T = int(edges.numel())
    g, i = gen.numpy().astype(np.float64), imp.numpy().astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        far_c = (i.sum() - np.cumsum(i)[:T]) / i.sum()
        frr_c = np.cumsum(g)[:T] / g.sum()
    gap = np.abs(far_c - frr_c)
    if np.all(np.isnan(gap)):
        eer = None
    else:
        at = int(np.nanargmin(gap))
        eer = dict(index=at, threshold=float(edges[at]), far=float(far_c[at]), frr=float(frr_c[at]),
                   eer=float((far_c[at] + frr_c[at]) / 2))
    return dict(edges=edges.cpu(), gen=gen, imp=imp, skipped=skipped, far=far_c, frr=frr_c, eer=eer,
                thresholds=[far_threshold(scores, row_lab, col_lab, f, own) for f in far])


# ----------------------------------------------------------------------------------------- stage ranks
class StageRanks(dict):
    """``stage_ranks``'s result: stage name -> dict(mate_col, mate_score, mate_rank: (Q,) host tensors as
    ``ops.mate_rank`` gives them; mate_entry / mate_subject: the column as an entry number / subject label, -1
    for none), beside ``stages`` (the names, in order) and ``mated`` (stage -> (Q,) bool)."""

    def recall(self, stage, K):
        """The fraction of the stage's mated probes whose mate survives a cut to the K best (rank < K); NaN
        without a mated probe."""
        r = self[stage]["mate_rank"]
        m = r >= 0
        return float((r[m] < int(K)).sum()) / int(m.sum()) if int(m.sum()) else float("nan")

    def cmc(self, stage, ks):
        return [self.recall(stage, k) for k in ks]


def _need_labels(what, probes, index):
    from .gallery import GalleryIndex
    from .sharded_gallery import ShardedGallery
    if isinstance(index, ShardedGallery) or isinstance(probes, ShardedGallery):
        raise FpmError("%s: not supported over a ShardedGallery (probe sets over shards are not built)" % what)
    if not isinstance(index, GalleryIndex) or not isinstance(probes, GalleryIndex):
        raise FpmError("%s: probes and index must be GalleryIndex objects (Net.enroll) with subject labels" % what)
    if probes.subject is None or index.subject is None:
        raise FpmError("%s: the probe set and the index need subject labels (enroll(subjects=...) or "
                       "GalleryIndex.set_subjects): a probe's mates are the entries of its label" % what)


def _own_positions(psel, sel):
    """Per probe the position of its own entry number in ``sel`` (the first), -1 where it is absent: host int32."""
    hit = psel.view(-1, 1) == sel.view(1, -1)
    return torch.where(hit.any(1), hit.to(torch.int8).argmax(1), torch.full((psel.numel(),), -1)).to(torch.int32)


def stage_ranks(net, probes, index, coarse="fused", exclude_self=False, probe_select=None, select=None,
                probe_chunk=None):
    """The rank of every probe's mate, stage by stage: every probe of ``probe_select`` against every entry of
    ``select`` (defaults: all), in chunks of ``probe_chunk`` probes (default: the most whose (chunk, entries) fp32
    matrix stays under ``STAGE_BYTES``), ``ops.mate_rank`` over each stage's scores -> ``StageRanks``:

      "desc"            ``ops.desc_score`` of the two sides' descriptors, when both hold them
      "coarse"          ``coarse_scores_many`` (``coarse``: its route)
      "coarse_subject"  the coarse scores fused per subject by max (``ops.group_scores``), ranked over subjects

    Labels are the sets' subject labels, mapped on the host to dense int32 places among the selection's distinct
    labels; a probe whose label is absent is non-mated (rank -1).  ``exclude_self`` (``probes is index``): the
    probe's own column is ignored at the entry stages and counts as -inf in the subject fuse -- leave-one-out
    evaluation of a gallery against itself; a probe that is its subject's only entry is then non-mated.  With
    one genuine entry per probe the mate survives a cut to K exactly when rank < K (``recall``); with several
    impressions the rank is the best one's (``ops.mate_rank``).  No query that ``identify_many`` refuses is made."""
    from . import gallery
    what = "stage_ranks"
    _need_labels(what, probes, index)
    if exclude_self and probes is not index:
        raise FpmError("%s: exclude_self needs the index as its own probe set (probes is index)" % what)
    psel = gallery._select_host(probes, probe_select, "%s (probe_select)" % what)
    sel = gallery._select_host(index, select, what)
    dev = index.device
    Qs, Gs = int(psel.numel()), int(sel.numel())
    gt = index.subject_groups(sel)
    labels = gt["labels"]                                        # the selection's distinct labels, ascending
    S = int(labels.numel())
    plab = probes.subject[psel]
    place = torch.searchsorted(labels, plab).clamp(max=S - 1)
    row_lab = torch.where(labels[place] == plab, place, torch.full_like(place, -1)).to(torch.int32)
    col_lab = gt["group"].to(torch.int32)                        # each selected entry's place
    own = _own_positions(psel, sel) if exclude_self else None
    row_sub = row_lab
    if own is not None:
        cnt = (gt["off"][1:] - gt["off"][:-1]).long()
        left = cnt[row_lab.clamp(min=0).long()] - (own >= 0).long()
        row_sub = torch.where((row_lab >= 0) & (left > 0), row_lab, torch.full_like(row_lab, -1))
    with_desc = probes.desc is not None and index.desc is not None
    stages = (["desc"] if with_desc else []) + ["coarse", "coarse_subject"]
    step = int(probe_chunk) if probe_chunk is not None else max(1, STAGE_BYTES // (4 * Gs))
    if step < 1:
        raise FpmError("%s: probe_chunk = %r below 1" % (what, probe_chunk))
    sel32 = sel.to(torch.int32)
    parts = {s: [] for s in stages}
    with torch.cuda.device(dev):
        col_d, sub_d, sel_d = col_lab.to(dev), torch.arange(S, dtype=torch.int32, device=dev), sel32.to(dev)
        for q0 in range(0, Qs, step):
            q1 = min(Qs, q0 + step)
            rl, rs = row_lab[q0:q1].to(dev), row_sub[q0:q1].to(dev)
            ow = None if own is None else own[q0:q1].to(dev)
            if with_desc:
                sc = ops.desc_score(probes.desc[psel[q0:q1].to(dev)].contiguous(), index.desc, sel_d, idx_host=sel32)
                parts["desc"].append(ops.mate_rank(sc, rl, col_d, ow))
            sc = gallery.coarse_scores_many(net, probes, index, probe_select=psel[q0:q1], select=sel, coarse=coarse)
            parts["coarse"].append(ops.mate_rank(sc, rl, col_d, ow))
            if ow is not None:
                cols = torch.arange(Gs, dtype=torch.int32, device=dev).view(1, Gs)
                sc = sc.masked_fill(cols == ow.view(-1, 1), float("-inf"))
            fused, _ = ops.group_scores(sc, gt["off_d"], gt["pos_d"], "max", off_host=gt["off"], pos_host=gt["pos"])
            parts["coarse_subject"].append(ops.mate_rank(fused, rs, sub_d))
    out = StageRanks(stages=stages, mated={})
    for s in stages:
        col, msc, rank = (torch.cat([p[i] for p in parts[s]]).cpu() for i in range(3))
        names = labels if s == "coarse_subject" else sel
        named = torch.where(col >= 0, names[col.clamp(min=0).long()], torch.full((Qs,), -1, dtype=torch.int64))
        out[s] = {"mate_col": col, "mate_score": msc, "mate_rank": rank,
                  "mate_subject" if s == "coarse_subject" else "mate_entry": named}
        out["mated"][s] = rank >= 0
    return out


# --------------------------------------------------------------------------------------- search funnel
def _host(t):
    return t.detach().cpu() if isinstance(t, torch.Tensor) else torch.as_tensor(t)


def funnel(results, probe_label, entry_subject, entries, own=None, by=None, score="cls_prob", ks=(1, 5, 10)):
    """The funnel of a probe-set query, read off ``identify_many``'s result dicts ``results`` (one per probe).
    ``probe_label`` (Q,): each probe's subject; ``entry_subject`` (G,): the gallery's labels by entry number;
    ``entries``: the entry numbers the query ran over (host); ``own`` (Q,) or None: each probe's own entry number
    (``exclude_self``), which is no mate; ``by``: the query's.  -> dict:

      probes   per probe a dict: ``mated`` (its label is among the searched entries, its own aside);
               ``in_prescreen`` / ``in_shortlist``: whether a mate (entry level: an entry of its label in
               ``pre_idx`` / ``short_idx``; ``by="subject"``: its label in ``short_subject``) is in the stage's
               list, None where the query had no such stage; ``rank``: the mate's rank in the exact ranking
               (``ops.mate_rank`` over ``subject_score`` with each row's ``subjects``, or over the exact
               ``score`` with each row's entries), -1 when it is in no list; ``match`` if the query decided
      stages   survival: the fraction of the mated probes whose mate is in the prescreen, in the shortlist, in
               the exact ranking (None for a stage the query had not)
      cmc      per k of ``ks`` the fraction of the mated probes with rank < k
      fnir, fpir   with ``threshold=``: mated probes whose ``match`` is not their subject over mated probes;
               non-mated probes with ``match != -1`` over non-mated probes (NaN over an empty class)"""
    Q = len(results)
    plab = _host(probe_label).to(torch.int64).view(-1)
    esub = _host(entry_subject).to(torch.int64).view(-1)
    ents = _host(entries).to(torch.int64).view(-1)
    ownh = None if own is None else _host(own).to(torch.int64).view(-1)
    if plab.numel() != Q or (ownh is not None and ownh.numel() != Q):
        raise FpmError("funnel: %d results, %d probe labels" % (Q, plab.numel()))
    subject = by == "subject"

    def mates_in(q, idx):
        idx = _host(idx).to(torch.int64).view(-1)
        hit = esub[idx] == plab[q]
        if ownh is not None:
            hit = hit & (idx != ownh[q])
        return hit

    rows, labs, per = [], [], []
    for q, r in enumerate(results):
        cand = ents if ownh is None else ents[ents != ownh[q]]
        d = dict(mated=bool((esub[cand] == plab[q]).any()), in_prescreen=None, in_shortlist=None)
        if "pre_idx" in r:
            d["in_prescreen"] = bool(mates_in(q, r["pre_idx"]).any())
        if subject:
            if "short_subject" in r:
                d["in_shortlist"] = bool((_host(r["short_subject"]).to(torch.int64) == plab[q]).any())
            rows.append(r["subject_score"].view(-1))
            labs.append((_host(r["subjects"]).to(torch.int64) == plab[q]).to(torch.int32))
        else:
            lst = r["short_idx"] if "short_idx" in r else cand
            hit = mates_in(q, lst)
            if "short_idx" in r:
                d["in_shortlist"] = bool(hit.any())
            rows.append(r[score].view(-1))
            lab = hit.to(torch.int32)
            if ownh is not None:
                lab = torch.where(_host(lst).to(torch.int64).view(-1) == ownh[q], torch.full_like(lab, -1), lab)
            labs.append(lab)
        if "match" in r:
            d["match"] = int(r["match"])
        per.append(d)
    if Q:
        # one matrix: the rows padded with ignored columns
        L = max(int(x.numel()) for x in rows)
        dev = rows[0].device
        mat = torch.zeros(Q, L, dtype=torch.float32, device=dev)
        lab = torch.full((Q, L), -1, dtype=torch.int32)
        for q in range(Q):
            n = int(rows[q].numel())
            if n != int(labs[q].numel()):
                raise FpmError("funnel: probe %d has %d exact scores for %d candidates" % (q, n, labs[q].numel()))
            mat[q, :n] = rows[q].to(torch.float32)
            lab[q, :n] = labs[q]
        _, _, rank = ops.mate_rank(mat, torch.ones(Q, dtype=torch.int32, device=dev), lab.to(dev))
        for q, v in enumerate(rank.cpu().tolist()):
            per[q]["rank"] = v
    mated = [d for d in per if d["mated"]]
    non = [d for d in per if not d["mated"]]
    frac = lambda n, m: n / m if m else float("nan")

    def survival(key):
        if not per or per[0][key] is None:
            return None
        return frac(sum(bool(d[key]) for d in mated), len(mated))

    out = dict(probes=per, mated=len(mated), non_mated=len(non),
               stages=dict(prescreen=survival("in_prescreen"), shortlist=survival("in_shortlist"),
                           exact=frac(sum(d["rank"] >= 0 for d in mated), len(mated))),
               cmc={int(k): frac(sum(0 <= d["rank"] < int(k) for d in mated), len(mated)) for k in ks})
    if per and "match" in per[0]:
        named = lambda d, q: d["match"] if subject else (int(esub[d["match"]]) if d["match"] >= 0 else -1)
        miss = sum(named(d, q) != int(plab[q]) for q, d in enumerate(per) if d["mated"])
        out.update(fnir=frac(miss, len(mated)), fpir=frac(sum(d["match"] != -1 for d in non), len(non)))
    return out


def search_report(net, probes, index, ks=(1, 5, 10), **query):
    """``net.identify_many(probes, index, **query)`` unchanged, and ``funnel`` over its results: which stage lost
    each probe's mate, the survival per stage, the CMC at ``ks`` and, with ``threshold=``, FNIR and FPIR.  Both
    sets carry subject labels.  -> ``funnel``'s dict with ``results`` (the query's own)."""
    from . import gallery
    what = "search_report"
    _need_labels(what, probes, index)
    results = net.identify_many(probes, index, **query)
    psel = gallery._select_host(probes, query.get("probe_select"), "%s (probe_select)" % what)
    sel = gallery._select_host(index, query.get("select"), what)
    rep = funnel(results, probes.subject[psel], index.subject, sel, own=psel if query.get("exclude_self") else None,
                 by=query.get("by"), score=query.get("score", "cls_prob"), ks=ks)
    rep["results"] = results
    return rep


# ------------------------------------------------------------------------- binary-classifier metrics
def _clf_curve(y, s):
    """Cumulative false and true positives at every distinct score, descending (a stable sort)."""
    order = np.argsort(s, kind="mergesort")[::-1]
    s, y = s[order], y[order]
    at = np.r_[np.where(np.diff(s))[0], y.size - 1]
    tps = np.cumsum(y, dtype=np.float64)[at]
    return 1 + at - tps, tps, s[at]


def _auc(x, y):
    dx = np.diff(x)
    sign = 1.0
    if np.any(dx < 0):
        if not np.all(dx <= 0):
            raise FpmError("verification_report: a curve that is neither rising nor falling")
        sign = -1.0
    return float(sign * np.sum(dx * (y[1:] + y[:-1]) / 2.0))


def verification_report(prob, label):
    """The reference's evaluate_binary_classifier.py:141-159 in float64 numpy, with no sklearn at run time:
    the ROC curve (distinct scores descending, collinear points dropped, a first point at threshold +inf), the
    EER threshold by nanargmin(|fnr - fpr|), predictions ``prob >= threshold``, then accuracy, precision, recall,
    F1, ROC AUC and PR AUC (trapezoids), FAR = fp / (fp + tn) and FRR = fn / (tp + fn).  ``prob`` (N,) scores,
    ``label`` (N,) in {0, 1}, both classes present.  -> dict of floats, the integer confusion counts ``tn``,
    ``fp``, ``fn``, ``tp``, ``eer_threshold`` and the curves ``fpr``, ``tpr``, ``thresholds``."""
    s = np.asarray(_host(prob).numpy() if isinstance(prob, torch.Tensor) else prob, dtype=np.float64).reshape(-1)
    y = np.asarray(_host(label).numpy() if isinstance(label, torch.Tensor) else label).reshape(-1)
    if s.size != y.size or s.size == 0:
        raise FpmError("verification_report: %d scores for %d labels" % (s.size, y.size))
    if np.isnan(s).any() or not np.isin(y, (0, 1)).all() or y.min() == y.max():
        raise FpmError("verification_report: scores must not be NaN, labels must be 0 / 1 with both present")
    y = y.astype(np.int64)
    fps, tps, thr = _clf_curve(y, s)
    if fps.size > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        rfps, rtps, rthr = fps[keep], tps[keep], thr[keep]
    else:
        rfps, rtps, rthr = fps, tps, thr
    rfps, rtps, rthr = np.r_[0.0, rfps], np.r_[0.0, rtps], np.r_[np.inf, rthr]
    fpr, tpr = rfps / rfps[-1], rtps / rtps[-1]
    fnr = 1 - tpr
    at = int(np.nanargmin(np.abs(fnr - fpr)))
    t = float(rthr[at])
    pred = s >= t
    tp, fp = int(np.sum(pred & (y == 1))), int(np.sum(pred & (y == 0)))
    fn, tn = int(np.sum(~pred & (y == 1))), int(np.sum(~pred & (y == 0)))
    ps = tps + fps
    prec = np.divide(tps, ps, out=np.zeros_like(tps), where=ps != 0)
    rec = tps / tps[-1]
    prec_curve, rec_curve = np.r_[prec[::-1], 1.0], np.r_[rec[::-1], 0.0]
    return dict(eer_threshold=t, eer_index=at, tn=tn, fp=fp, fn=fn, tp=tp,
                accuracy=(tp + tn) / y.size, precision=tp / (tp + fp) if tp + fp else 0.0,
                recall=tp / (tp + fn) if tp + fn else 0.0, f1=2 * tp / (2 * tp + fp + fn) if tp + fp + fn else 0.0,
                roc_auc=_auc(fpr, tpr), pr_auc=_auc(rec_curve, prec_curve),
                far=fp / (fp + tn) if fp + tn else 0.0, frr=fn / (tp + fn) if tp + fn else 0.0,
                fpr=fpr, tpr=tpr, thresholds=rthr)

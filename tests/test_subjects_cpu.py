"""Subject-level 1:N search, host side (no GPU): the statement of ``ops.group_scores`` (max, gbest and the
fixed-order mean), the index's subject labels and group tables, ``save`` / ``load``, the refusals, and the
query layer's host-side stages (the shortlist stage and the probe-set exact stage's pair lists) against
plain Python loops.

Mean bound: against float64 a group's mean may differ by ``(cnt + 1) * 2^-24 * sum|x| / cnt`` -- the
first-order bound of any fp32 summation order (cnt - 1 additions on a path at most; here far fewer)
plus the rounding of the divide.  The statement is held to it on every finite group below, and an
independent lane-by-lane loop in numpy pins its order bit for bit."""
import math
import types

import numpy as np
import pytest
import torch

from fpm import _lib, gallery, ops
from fpm.gallery import GalleryIndex
from test_compact_index_cpu import hand_index

COUNTS = (1, 15, 16, 17, 63, 64, 65, 1024, 1025, 4097)
QNAN = 0x7FC00000


def _bits(t):
    return t.contiguous().view(torch.int32)


def _strided(s, extra=9):
    """The same values as a view whose row stride exceeds G."""
    wide = torch.zeros(s.shape[0], s.shape[1] + extra)
    wide[:, 4:4 + s.shape[1]] = s
    return wide[:, 4:4 + s.shape[1]]


def _csr(groups):
    off = torch.tensor([0] + list(np.cumsum([len(g) for g in groups])), dtype=torch.int32)
    pos = torch.tensor([q for g in groups for q in g], dtype=torch.int32)
    return off, pos


def counts_case(P=3, seed=1):
    """Groups of COUNTS entries and an empty one, at scattered positions that leave 37 of the row out."""
    gen = torch.Generator().manual_seed(seed)
    G = sum(COUNTS) + 37
    perm = torch.randperm(G, generator=gen).tolist()
    groups, at = [], 0
    for i, c in enumerate(COUNTS):
        if i == 4:
            groups.append([])
        groups.append(perm[at:at + c])
        at += c
    return _strided(torch.randn(P, G, generator=gen)), groups


def special_case():
    nan, inf = float("nan"), float("inf")
    row = torch.tensor([[1.0, 1.0, nan, -0.0, 0.0, inf, -inf, nan, nan, 2.0, -inf, inf, 3.0, 3.0, 0.5]])
    groups = [[1, 0], [2, 0], [3, 4], [4, 3], [5, 6], [7, 8, 2], [5, 11], [9, 2], [], [13, 12, 9], [6, 10], [3], [14]]
    best = [0, 0, 4, 4, 5, 2, 5, 9, -1, 12, 6, 3, 14]
    return _strided(row), groups, best


def all_cases():
    """name -> (scores (P, G) with row stride > G, list of groups): shared by the GPU test."""
    gen = torch.Generator().manual_seed(2)
    out = {"counts-P3": counts_case(3), "counts-P1": counts_case(1, seed=4)}
    out["singletons"] = (_strided(torch.randn(1, 1000, generator=gen)), [[i] for i in range(1000)])
    out["one-group"] = (_strided(torch.randn(3, 5000, generator=gen)), [torch.randperm(5000, generator=gen).tolist()])
    s, groups, _ = special_case()
    out["special"] = (s, groups)
    return out


_CASES = {}


def cases():
    if not _CASES:
        _CASES.update(all_cases())
    return _CASES


def per_row_case():
    """Three rows, each with its own structure; rows 0 and 2 carry the shared structure of counts-P3 (cut
    to its first 7 groups), row 1 another -> (scores, off (3, S + 1), pos (3, L), shared groups)."""
    s, groups = cases()["counts-P3"]
    shared = groups[:7]
    gen = torch.Generator().manual_seed(6)
    perm = torch.randperm(s.shape[1], generator=gen).tolist()
    other, at = [], 0
    for c in (5, 0, 40, 1, 17, 2, 300):
        other.append(perm[at:at + c])
        at += c
    offs, poss = zip(*[_csr(g) for g in (shared, other, shared)])
    L = max(int(p.numel()) for p in poss) + 3
    pos = torch.zeros(3, L, dtype=torch.int32)
    for i, p in enumerate(poss):
        pos[i, :p.numel()] = p
    return s, torch.stack(offs), pos, shared, other


def loop_reference(s, groups):
    """gbest and the max by a plain Python loop over ``rank_key``."""
    key = ops.rank_key(s)
    P = s.shape[0]
    best = torch.full((P, len(groups)), -1, dtype=torch.int32)
    val = torch.full((P, len(groups)), float("nan"))
    for p in range(P):
        krow = key[p].tolist()
        for g, members in enumerate(groups):
            if members:
                q = max(members, key=lambda m: krow[m])
                best[p, g], val[p, g] = q, s[p, q]
    return val, best


def lane_mean(x):
    """The mean's order, lane by lane in numpy fp32 (independent of the torch statement)."""
    c = len(x)
    W = 64 if c > 1024 else 16
    lanes = [np.float32(0.0)] * W
    for j, v in enumerate(x):
        lanes[j % W] = np.float32(lanes[j % W] + np.float32(v))
    m = W // 2
    while m:
        lanes = [np.float32(lanes[t] + lanes[t ^ m]) for t in range(W)]
        m //= 2
    return np.float32(lanes[0] / np.float32(c))


# ----------------------------------------------------------------------------- the statement: max
@pytest.mark.parametrize("name", sorted(all_cases()))
def test_group_max_and_best_against_the_loop(name):
    s, groups = cases()[name]
    assert s.stride(0) > s.shape[1]
    off, pos = _csr(groups)
    val, best = ops.group_scores(s, off, pos, "max")
    rv, rb = loop_reference(s, groups)
    assert best.dtype == torch.int32 and tuple(best.shape) == (s.shape[0], len(groups))
    assert torch.equal(best, rb) and torch.equal(_bits(val), _bits(rv))
    # gbest is the same under the mean
    assert torch.equal(ops.group_scores(s, off, pos, "mean")[1], rb)


def test_special_values():
    s, groups, best = special_case()
    off, pos = _csr(groups)
    val, gb = ops.group_scores(s, off, pos, "max")
    assert gb[0].tolist() == best
    assert _bits(val)[0, 2].item() == 0 and _bits(val)[0, 3].item() == 0        # +0 beats -0, whatever the order
    assert bool(torch.isnan(val[0, 5])) and bool(torch.isnan(val[0, 8]))
    mean, gb = ops.group_scores(s, off, pos, "mean")
    assert gb[0].tolist() == best
    want = [1.0, None, 0.0, 0.0, None, None, float("inf"), None, None, 8.0 / 3, float("-inf"), -0.0, 0.5]
    for g, w in enumerate(want):
        if w is None:
            assert _bits(mean)[0, g].item() == QNAN, g                           # NaN propagates, canonical bits
        else:
            assert mean[0, g].item() == pytest.approx(w, rel=1e-6), g
    assert _bits(mean)[0, 11].item() == 0                                        # +0.0 + -0.0: the lane starts at +0.0


# ---------------------------------------------------------------------------- the statement: mean
@pytest.mark.parametrize("name", ["counts-P3", "counts-P1", "singletons", "one-group"])
def test_group_mean_against_float64_and_the_lane_loop(name):
    s, groups = cases()[name]
    off, pos = _csr(groups)
    mean, _ = ops.group_scores(s, off, pos, "mean")
    for g, members in enumerate(groups):
        if not members:
            assert _bits(mean)[:, g].tolist() == [QNAN] * s.shape[0]
            continue
        x = s[:, members].double()
        cnt = len(members)
        bound = (cnt + 1) * 2.0 ** -24 * x.abs().sum(1) / cnt
        err = (mean[:, g].double() - x.mean(1)).abs()
        assert bool((err <= bound).all()), (name, g, cnt, float(err.max()), float(bound.min()))
    # the order itself, bit for bit, on row 0 (every group of the count cases; a sample of the others)
    for g in range(len(groups)) if name.startswith("counts") else range(0, len(groups), 97):
        if groups[g]:
            want = lane_mean(s[0, groups[g]].numpy())
            assert _bits(mean)[0, g].item() == int(want.view(np.int32)), (name, g)


def test_shared_and_per_row_structures_agree():
    s, off, pos, shared, other = per_row_case()
    so, sp = _csr(shared)
    for fuse in ops.GROUP_FUSE:
        val, gb = ops.group_scores(s, off, pos, fuse)
        rv, rb = ops.group_scores(s, so, sp, fuse)
        for p in (0, 2):
            assert torch.equal(gb[p], rb[p]) and torch.equal(_bits(val[p]), _bits(rv[p])), (fuse, p)
        ov, ob = ops.group_scores(s[1:2], *_csr(other), fuse)
        assert torch.equal(gb[1], ob[0]) and torch.equal(_bits(val[1]), _bits(ov[0])), fuse
    # a group's result does not depend on the launch: alone (S = 1, P = 1) and inside the whole
    for g in (0, 3, 6):
        av, ab = ops.group_scores(s[2:3], *_csr([shared[g]]), "mean")
        assert torch.equal(_bits(av[0]), _bits(val[2, g:g + 1])) and int(ab[0, 0]) == int(gb[2, g])


# --------------------------------------------------------------------- group tables and the container
def labelled_index(labels):
    """An index of len(labels) one-keypoint entries on the CPU "device"."""
    G = len(labels)
    gen = torch.Generator().manual_seed(8)
    z = torch.zeros(0, dtype=torch.int32)
    return GalleryIndex(torch.randn(G, 768, generator=gen), torch.arange(G + 1), torch.ones(G, dtype=torch.int32), z, z,
                        torch.zeros(0, 2), torch.zeros(G + 1, dtype=torch.int64), torch.rand(G, 512, generator=gen), None,
                        "f32", 1, "abcd", subject=labels)


def _check_tables(t, labels_of_selection):
    want = {}
    for p, lab in enumerate(labels_of_selection):
        want.setdefault(int(lab), []).append(p)
    assert t["labels"].dtype == torch.int64 and t["labels"].tolist() == sorted(want)
    assert t["off"].dtype == torch.int32 and t["pos"].dtype == torch.int32
    got = {int(lab): t["pos"][int(t["off"][s]):int(t["off"][s + 1])].tolist() for s, lab in enumerate(t["labels"])}
    assert got == want                                       # ascending positions inside a group
    assert [int(t["labels"][g]) for g in t["group"]] == [int(v) for v in labels_of_selection]
    for k in ("off", "pos", "labels"):
        assert torch.equal(t[k + "_d"], t[k])


def test_subject_groups_against_a_dict_of_lists():
    labels = [7, 3, 7, 0, 3, 7, 11, 0, 5, 3, 7, 2]
    index = labelled_index(labels)
    assert index.subject.dtype == torch.int64 and index.subject.tolist() == labels
    plain = index.nbytes()
    t = index.subject_groups()
    _check_tables(t, labels)
    assert index.subject_groups() is t                       # the last selection's tables are kept
    assert index.nbytes() == plain + sum(t[k].numel() * t[k].element_size() for k in ("labels_d", "off_d", "pos_d"))
    sel = [10, 1, 4, 6, 0, 9, 3, 5]                          # a permuted sub-selection, no entry twice
    t2 = index.subject_groups(sel)
    _check_tables(t2, [labels[e] for e in sel])
    assert index.subject_groups(torch.tensor(sel)) is t2 and index.subject_groups() is not t
    index.set_subjects([1] * 12)                             # relabelling drops the cached tables
    assert index._groups is None and index.nbytes() == plain
    assert index.subject_groups()["labels"].tolist() == [1] and index.subject_groups()["off"].tolist() == [0, 12]


def test_set_subjects_checks():
    index = hand_index("f32")
    assert index.subject is None
    with pytest.raises(_lib.FpmError, match="no subject labels"):
        index.subject_groups()
    for bad, msg in (([0, 1], "one label per entry"), ([[0, 1, 2]], "one label per entry"),
                     ([0.0, 1.0, 2.0], "must be integers"), ([0, -1, 2], "negative subject label"),
                     ([True, False, True], "must be integers")):
        with pytest.raises(_lib.FpmError, match=msg):
            index.set_subjects(bad)
    assert index.subject is None
    given = torch.tensor([4, 4, 9], dtype=torch.int32)
    index.set_subjects(given)
    given[0] = 77                                            # the index keeps its own copy
    assert index.subject.dtype == torch.int64 and index.subject.tolist() == [4, 4, 9]
    index.set_subjects(None)
    assert index.subject is None
    a = (index.y, index.row_off, index.n, index.src, index.dst, index.pseudo, index.edge_off, index.w, None, "f32", 1, "x")
    with pytest.raises(_lib.FpmError, match="one label per entry"):
        GalleryIndex(*a, subject=[1, 2])


@pytest.mark.parametrize("layout", ["f32", "f32+bf16", "bf16+host"])
def test_labels_round_trip_through_save_and_load(tmp_path, layout):
    index = hand_index(layout)
    index.set_subjects([5, 0, 5])
    path = str(tmp_path / "gallery.pt")
    index.save(path)
    raw = torch.load(path, map_location="cpu", weights_only=True)
    assert raw["format"] == (1 if layout == "f32" else 2) and raw["subject"].tolist() == [5, 0, 5]
    back = GalleryIndex.load(path, "cpu")
    assert back.subject.dtype == torch.int64 and torch.equal(back.subject, index.subject) and back.layout == layout
    for k in ("y", "row_off", "n", "src", "dst", "pseudo", "edge_off", "w", "P"):
        assert torch.equal(getattr(back, k), getattr(index, k)), k
    assert back.subject_groups()["off"].tolist() == [0, 1, 3]


def test_unlabelled_index_saves_what_it_saved_before(tmp_path):
    path = str(tmp_path / "gallery.pt")
    hand_index("f32").save(path)
    raw = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(raw) == sorted(["format", "y", "row_off", "n", "src", "dst", "pseudo", "edge_off", "w", "sc_mode",
                                  "pack_gen", "weights_id", "P"]) and raw["format"] == 1
    assert GalleryIndex.load(path, "cpu").subject is None
    hand_index("bf16+host").save(path)
    raw2 = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(raw2) == sorted(list(raw) + ["layout", "y16"]) and raw2["format"] == 2


# ------------------------------------------------------------- the query stages against plain loops
STAGE_LABELS = [3, 1, 3, 0, 1, 3, 5]                         # subjects of 1, 2, 3 and 1 impressions
STAGE_SELECTIONS = {"in-order": [0, 1, 2, 3, 4, 5, 6], "permuted": [4, 0, 6, 2, 5, 1, 3]}


def stage_case(sel, with_own):
    """Q = 3 probes over the selection ``sel`` of the 7 labelled entries -> (coarse matrix (3, 7) by
    position in the selection, own mask or None).  Row 0 carries a tie at the top between entry 1
    (subject 1) and entry 6 (the singleton subject 5), row 2 a NaN at entry 3 (the singleton subject 0);
    ``own`` removes entry 6 for probe 1: the only entry of its subject."""
    gen = torch.Generator().manual_seed(11)
    by_entry = torch.randn(3, 7, generator=gen)
    by_entry[0, 1] = by_entry[0, 6] = 9.0
    by_entry[2, 3] = float("nan")
    call = by_entry[:, sel].contiguous()
    own = None
    if with_own:
        own = torch.zeros(3, 7, dtype=torch.bool)
        own[1, sel.index(6)] = True
    return call, own


def _best_first(vals):
    """Indices of a list of floats, best first: descending, ties to the lower index, NaN after every
    number (-inf included), NaNs by index."""
    return sorted(range(len(vals)), key=lambda i: (math.isnan(vals[i]), 0.0 if math.isnan(vals[i]) else -vals[i], i))


def shortlist_loop(call, sel, M, own, subject, impressions):
    """The shortlist stage by a plain loop over a dict of lists -> per probe (entry list, offsets or None,
    names, coarse scores as (probe row, position) of ``call`` or None for -inf)."""
    groups = {}
    for p, e in enumerate(sel):
        groups.setdefault(STAGE_LABELS[e], []).append(p)
    labels = sorted(groups)
    out = []
    for q in range(call.shape[0]):
        gone = [own is not None and bool(own[q, p]) for p in range(len(sel))]
        vals = [float("-inf") if gone[p] else float(call[q, p]) for p in range(len(sel))]
        if not subject:
            top = _best_first(vals)[:min(M, len(sel) - (own is not None))]
            out.append(([sel[p] for p in top], None, [sel[p] for p in top], [vals[p] for p in top]))
            continue
        best = {lab: groups[lab][_best_first([vals[p] for p in groups[lab]])[0]] for lab in labels}
        top = _best_first([vals[best[lab]] for lab in labels])[:min(M, len(labels))]
        ents, offs = [], [0]
        for s in top:
            members = groups[labels[s]] if impressions == "all" else [best[labels[s]]]
            ents += [sel[p] for p in members if not gone[p]]
            offs.append(len(ents))
        out.append((ents, offs, [labels[s] for s in top], [vals[best[labels[s]]] for s in top]))
    return out


def _same_floats(t, want):
    got = t.tolist()
    return len(got) == len(want) and all((math.isnan(a) and math.isnan(b)) or a == b for a, b in zip(got, want))


@pytest.mark.parametrize("with_own", [False, True])
@pytest.mark.parametrize("M", [1, 3, 4])
@pytest.mark.parametrize("order", sorted(STAGE_SELECTIONS))
def test_shortlist_stage_against_the_loop(order, M, with_own, monkeypatch):
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("the library was called"))
    sel = STAGE_SELECTIONS[order]
    call, own = stage_case(sel, with_own)
    index = labelled_index(STAGE_LABELS)
    sel_t = torch.tensor(sel)
    gt = index.subject_groups(sel_t)
    emptied = False
    for subject, impressions in ((False, "all"), (True, "all"), (True, "best")):
        ents, offs, names, csc = gallery._shortlist(call, sel_t, M, own, gt if subject else None, impressions)
        want = shortlist_loop(call, sel, M, own, subject, impressions)
        assert len(ents) == 3 and names.dtype == torch.int64 and csc.dtype == torch.float32
        assert (offs is None) == (not subject)
        for q, (w_ents, w_offs, w_names, w_csc) in enumerate(want):
            where = (order, M, with_own, subject, impressions, q)
            assert ents[q].dtype == torch.int64 and ents[q].tolist() == w_ents, where
            assert names[q].tolist() == w_names, where
            assert _same_floats(csc[q], w_csc), where
            if subject:
                assert offs[q].tolist() == w_offs and len(w_offs) == len(w_names) + 1, where
                emptied |= any(a == b for a, b in zip(w_offs, w_offs[1:]))
    # leave-one-out: the emptied singleton subject keeps an empty range in the offsets (once the shortlist
    # is long enough to reach it: its fused score is -inf)
    assert emptied == (with_own and M == 4)


@pytest.mark.parametrize("impressions", ["all", "best"])
@pytest.mark.parametrize("with_own", [False, True])
def test_subject_entry_lists_against_the_loop(with_own, impressions):
    """``_subject_entry_lists`` alone, fed the loop's own ranking: positions and offsets."""
    sel = STAGE_SELECTIONS["permuted"]
    call, own = stage_case(sel, with_own)
    gt = labelled_index(STAGE_LABELS).subject_groups(torch.tensor(sel))
    labels = gt["labels"].tolist()
    for M in (1, 3, 4):
        want = shortlist_loop(call, sel, M, own, True, impressions)
        spos = torch.tensor([[labels.index(lab) for lab in w[2]] for w in want], dtype=torch.int32)
        masked = call if own is None else call.masked_fill(own, float("-inf"))
        best = ops.group_scores(masked, gt["off"], gt["pos"], "max")[1] if impressions == "best" else None
        lists = gallery._subject_entry_lists(gt, spos, best, own)
        for (p, so), (w_ents, w_offs, _, _) in zip(lists, want):
            assert [sel[int(i)] for i in p] == w_ents and so.tolist() == w_offs, (M, with_own, impressions)


def test_exact_stage_pair_lists_and_slices(monkeypatch):
    """The probe-set exact stage on ragged lists (3, 1 and 2 pairs, ``group_pairs`` = 4): each group's
    pair list and each probe's slice of the batch's outputs, with the forward replaced by a stub."""
    psel = torch.tensor([5, 2, 7])
    ents = [torch.tensor([10, 11, 12]), torch.tensor([20]), torch.tensor([30, 31])]
    probes = types.SimpleNamespace(n=torch.tensor([9, 9, 4, 9, 9, 6, 9, 5], dtype=torch.int32))   # probes 5, 2, 7: 6, 4, 5
    seen = []

    def run_pairs(net, pset, index, pairs, chunks):
        assert pset is probes and index == "index" and chunks == 3
        seen.append(pairs.tolist())
        B = pairs.shape[0]
        code = (pairs[:, 0] * 100 + pairs[:, 1]).float()
        return dict(cls_prob=code, s=code.view(B, 1, 1).expand(B, 2, 3), ks_loss=torch.tensor(7.0),
                    other=torch.arange(B + 1))

    monkeypatch.setattr(gallery, "_run_pairs", run_pairs)
    outs, rows = gallery._exact_many("net", probes, "index", psel, ents, "cls_prob", 3, 4)
    # ascending keypoint count: probe 2 (4), probe 7 (5), probe 5 (6); 1 + 2 pairs fit 4, the 3 of probe 5 do not
    assert seen == [[[2, 20], [7, 30], [7, 31]], [[5, 10], [5, 11], [5, 12]]]
    assert [o["group"] for o in outs] == [(1, 0, 3), (0, 0, 1), (0, 1, 3)]
    for q, (o, row) in enumerate(zip(outs, rows)):
        want = [float(psel[q]) * 100 + e for e in ents[q].tolist()]
        assert row.tolist() == want and o["cls_prob"].tolist() == want
        assert tuple(o["s"].shape) == (len(want), 2, 3) and o["s"][:, 0, 0].tolist() == want
        assert o["ks_loss"].dim() == 0 and set(o) == {"cls_prob", "s", "ks_loss", "other", "group"}
        # a tensor that is not batch-sized is passed on whole (both batches have three pairs)
        assert o["other"].tolist() == [0, 1, 2, 3]
    # lists of equal length (the entry-level query): the same slicing, one group when it fits
    del seen[:]
    outs, rows = gallery._exact_many("net", probes, "index", psel, [e[:1] for e in ents], "cls_prob", 3, 4)
    assert seen == [[[2, 20], [7, 30], [5, 10]]] and [o["group"] for o in outs] == [(0, 2, 3), (0, 0, 1), (0, 1, 2)]


# ---------------------------------------------------------------------------------------- refusals
def test_refusals(monkeypatch):
    def trap(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", trap)
    s = torch.zeros(2, 10)
    off, pos = _csr([[0, 1], [5]])
    ops.group_scores(s, off, pos)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    for kw, msg in ((dict(off=i32([1, 2, 3])), "start at 0"), (dict(off=i32([0, 3, 2])), "must not fall"),
                    (dict(off=i32([0, 2, 4])), "pos holds 3"), (dict(pos=i32([0, 10, 5])), r"outside \[0, 10\)"),
                    (dict(pos=i32([0, -1, 5])), r"outside \[0, 10\)"), (dict(off=off.long()), "off must be a int32"),
                    (dict(pos=pos.long()), "pos must be a int32"), (dict(fuse="median"), "fuse must be one of"),
                    (dict(scores=s.double()), "fp32"), (dict(scores=torch.zeros(65536, 1), pos=i32([0, 0, 0])), "65535 rows"),
                    (dict(off=torch.stack([off, off]), pos=pos), "shared structure"),
                    (dict(off=torch.stack([off] * 3), pos=torch.stack([pos] * 3)), "per-row structures"),
                    (dict(off_host=i32([0, 1, 3, 3])), "host copies")):
        a = dict(scores=s, off=off, pos=pos, fuse="max")
        a.update(kw)
        with pytest.raises(_lib.FpmError, match=msg):
            ops.group_scores(a.pop("scores"), a.pop("off"), a.pop("pos"), **a)
    # a per-row structure's padding is not read: only the used positions are checked
    ops.group_scores(s, torch.stack([off, off]), torch.tensor([[0, 1, 5, 99], [0, 1, 5, -7]], dtype=torch.int32))

    net = types.SimpleNamespace(training=False, use_graphs=False, dtype_mode="f32")   # refused before the net is asked
    plain, lab = hand_index("f32"), hand_index("f32")
    lab.set_subjects([0, 0, 1])
    probe = {"n": 3}
    for call in (lambda **kw: gallery.identify(net, probe, kw.pop("index", lab), **kw),
                 lambda **kw: gallery.identify_many(net, lab, kw.pop("index", lab), **kw)):
        with pytest.raises(_lib.FpmError, match="needs subject labels"):
            call(index=plain, by="subject")
        with pytest.raises(_lib.FpmError, match="fuse must be one of"):
            call(by="subject", fuse="sum")
        with pytest.raises(_lib.FpmError, match="impressions must be one of"):
            call(by="subject", impressions="first")
        with pytest.raises(_lib.FpmError, match="without by='subject'"):
            call(impressions="best", shortlist=2)
        with pytest.raises(_lib.FpmError, match="by must be None or 'subject'"):
            call(by="entry")
        with pytest.raises(_lib.FpmError, match="needs a shortlist"):
            call(by="subject", impressions="best")
    # enrolment checks the labels before any GPU work (the stand-in net has no weights to pack)
    graphs = [{"n": 3}, {"n": 4}]
    with pytest.raises(_lib.FpmError, match="one label per entry"):
        gallery.enroll(net, graphs, "cpu", subjects=[0])
    with pytest.raises(_lib.FpmError, match="negative subject label"):
        gallery.enroll_keypoints(net, torch.zeros(2, 4, 2), [3, 4], None, None, subjects=[0, -3])

"""Search evaluation on the GPU: ``ops.mate_rank``, ``ops.score_census`` and ``ops.score_select`` against their host
statements (bit for bit; all three are integer-exact), their independence of how the matrix is cut, the refusals
(nothing is launched), the C-ABI, and ``evaluate.stage_ranks`` / ``search_report`` end to end on the planted gallery
of ``test_shortlist_gpu`` (40 entries, three probes with one mate each, descriptors on).
"""
import ctypes

import pytest
import torch

import fpm
from fpm import _lib, evaluate, ops
from fpm.sharded_gallery import ShardedGallery
from test_evaluate_cpu import QNAN, eval_case
from test_shortlist_cpu import state_dicts
from test_shortlist_gpu import MATES, _net, planted

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GS = (1, 63, 64, 65, 257, 5000)            # 5000: more than one slice of 4096 columns, several workgroups a row
PS = (1, 3, 70)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(dev, host, what=None):
    assert len(dev) == len(host)
    for d, h in zip(dev, host):
        assert d.dtype == h.dtype and tuple(d.shape) == tuple(h.shape), what
        assert torch.equal(_bits(d.cpu()), _bits(h)), what


def _to(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


@pytest.fixture(scope="module", params=GS)
def case(request):
    """One 70-row case per G (shared and per-row labels) with its host results, computed once."""
    G = request.param
    s, row, col, own = eval_case(70, G, 1000 + G)
    _, _, col2, _ = eval_case(70, G, 2000 + G, per_row=True)
    return G, s, row, col, col2, own


# ---------------------------------------------------------------------------------- kernels vs host
def test_mate_rank_device_equals_host(case):
    G, s, row, col, col2, own = case
    s_d, row_d, col_d, col2_d, own_d = _to(s, row, col, col2, own)
    full = ops.mate_rank(s_d, row_d, col_d, own_d)
    assert all(t.device == DEV for t in full)
    _same(full, ops.mate_rank(s, row, col, own), G)
    for P in PS:
        for c, c_d in ((col, col_d), (col2[:P].contiguous(), col2_d[:P].contiguous())):
            for o, o_d in ((own[:P], own_d[:P].contiguous()), (None, None)):
                _same(ops.mate_rank(s_d[:P], row_d[:P].contiguous(), c_d, o_d),
                      ops.mate_rank(s[:P], row[:P], c, o), (P, G))
    # a row alone equals its row of the 70-row launch
    for p in (0, 37, 69):
        alone = ops.mate_rank(s_d[p:p + 1], row_d[p:p + 1].contiguous(), col_d, own_d[p:p + 1].contiguous())
        _same(alone, [t[p:p + 1].cpu() for t in full], (p, G))
    # a strided view (row stride > G)
    wide = torch.zeros(70, G + 9)
    wide[:, 4:4 + G] = s
    _same(ops.mate_rank(wide.to(DEV)[:, 4:4 + G], row_d, col_d, own_d), [t.cpu() for t in full], G)


@pytest.mark.parametrize("T", [1, 2, 4095])
def test_score_census_device_equals_host(case, T):
    G, s, row, col, col2, own = case
    edges = torch.linspace(-1.5, 1.0, T) if T > 1 else torch.tensor([0.0])      # -1, 0 and 1 sit on or by edges
    s_d, row_d, col_d, col2_d, own_d, e_d = _to(s, row, col, col2, own, edges)
    full = ops.score_census(s_d, row_d, col_d, e_d, own_d)
    assert all(t.device == DEV and t.dtype == torch.int64 for t in full)
    assert int(sum(t.sum() for t in full)) == 70 * G
    _same(full, ops.score_census(s, row, col, edges, own), (G, T))
    for P in (1, 3):
        _same(ops.score_census(s_d[:P], row_d[:P].contiguous(), col2_d[:P].contiguous(), e_d),
              ops.score_census(s[:P], row[:P], col2[:P].contiguous(), edges), (P, G, T))
    # the census of a matrix is the sum of the censuses of its two halves
    a = ops.score_census(s_d[:31], row_d[:31].contiguous(), col_d, e_d, own_d[:31].contiguous())
    b = ops.score_census(s_d[31:], row_d[31:].contiguous(), col_d, e_d, own_d[31:].contiguous())
    _same([x + y for x, y in zip(a, b)], [t.cpu() for t in full], (G, T))
    wide = torch.zeros(70, G + 9)
    wide[:, 4:4 + G] = s
    _same(ops.score_census(wide.to(DEV)[:, 4:4 + G], row_d, col_d, e_d, own_d), [t.cpu() for t in full], (G, T))


@pytest.mark.parametrize("cls", ops.SCORE_CLASSES)
def test_score_select_device_equals_host(case, cls):
    G, s, row, col, col2, own = case
    s_d, row_d, col_d, col2_d, own_d = _to(s, row, col, col2, own)
    _, n = ops.score_select(s, row, col, cls, 1, own)
    ks = sorted({1, 2, max(1, n // 3), max(1, n // 2), max(1, n - 1), max(1, n), n + 1})
    for k in ks:
        hv, hn = ops.score_select(s, row, col, cls, k, own)
        dv, dn = ops.score_select(s_d, row_d, col_d, cls, k, own_d)
        assert dn == hn == n and int(_bits(dv.view(1))[0]) == int(_bits(hv.view(1))[0]), (G, cls, k)
    assert int(_bits(ops.score_select(s_d, row_d, col_d, cls, n + 1, own_d)[0].view(1))[0]) == QNAN
    for P in (1, 3):
        k = 1 + P
        hv, hn = ops.score_select(s[:P], row[:P], col2[:P].contiguous(), cls, k)
        dv, dn = ops.score_select(s_d[:P], row_d[:P].contiguous(), col2_d[:P].contiguous(), cls, k)
        assert dn == hn and int(_bits(dv.view(1))[0]) == int(_bits(hv.view(1))[0]), (P, G, cls)
    # distinct values too (all 32 bits of the radix search matter), through a strided view
    g = torch.Generator().manual_seed(G)
    x = torch.randn(70, G, generator=g) * torch.tensor([1e-30, 1.0, 1e30])[torch.randint(0, 3, (70, G), generator=g)]
    wide = torch.zeros(70, G + 9)
    wide[:, 4:4 + G] = x
    _, n = ops.score_select(x, row, col, cls, 1)
    for k in sorted({1, max(1, n // 2), max(1, n)}):
        hv, hn = ops.score_select(x, row, col, cls, k)
        dv, dn = ops.score_select(wide.to(DEV)[:, 4:4 + G], row_d, col_d, cls, k)
        assert dn == hn and int(_bits(dv.view(1))[0]) == int(_bits(hv.view(1))[0]), (G, cls, k)


def test_far_threshold_on_device():
    s, row, col, own = eval_case(70, 5000, 77, specials=False)
    s = s + torch.randn(70, 5000, generator=torch.Generator().manual_seed(1)).round(decimals=1)     # ties
    host = evaluate.far_threshold(s, row, col, 1e-3, own)
    assert evaluate.far_threshold(*_to(s, row, col), 1e-3, own.to(DEV)) == host
    assert host["false_accepts"] <= host["k"] == int(1e-3 * host["impostors"])


# ---------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(monkeypatch):
    s, row, col, own = _to(*eval_case(3, 9, 1))
    edges = torch.tensor([0.0, 1.0], device=DEV)

    def boom(*a, **k):
        raise AssertionError("a launch before the refusal")

    monkeypatch.setattr(_lib, "call", boom)
    bad = [
        (lambda: ops.mate_rank(s.double(), row, col), "fp32"),
        (lambda: ops.mate_rank(s, row.long(), col), "int32"),
        (lambda: ops.mate_rank(s, row.cpu(), col), "is on"),
        (lambda: ops.mate_rank(s, row, col, own.cpu()), "is on"),
        (lambda: ops.mate_rank(s, row, col[:5].contiguous()), "col_lab of shape"),
        (lambda: ops.mate_rank(s, row, col, own[:2].contiguous()), "own"),
        (lambda: ops.score_census(s, row, col, torch.tensor([1.0, 0.0], device=DEV)), "ascending"),
        (lambda: ops.score_census(s, row, col, torch.tensor([0.0, float("inf")], device=DEV)), "finite"),
        (lambda: ops.score_census(s, row, col, torch.zeros(0, device=DEV)), "outside"),
        (lambda: ops.score_census(s, row, col, torch.arange(4096.0, device=DEV)), "outside"),
        (lambda: ops.score_census(s, row, col, edges.cpu()), "is on"),
        (lambda: ops.score_select(s, row, col, "impostor", 0), "k = 0"),
        (lambda: ops.score_select(s, row, col, "mate", 1), "cls"),
        (lambda: evaluate.far_threshold(s, row, col, 1.5), "outside"),
    ]
    for call, msg in bad:
        with pytest.raises(_lib.FpmError, match=msg):
            call()


# ------------------------------------------------------------------------------------------- C-ABI
def test_c_abi_entry_points():
    lib = _lib.load()
    P = ctypes.c_void_p
    st = P(torch.cuda.current_stream(DEV).cuda_stream)
    s, row, col, own = eval_case(5, 4500, 3)
    s_d, row_d, col_d, own_d = _to(s, row, col, own)
    ptr = lambda t: P(t.data_ptr())
    common = (ptr(s_d), 4500, 5, 4500, ptr(row_d), ptr(col_d), 0, ptr(own_d))

    mc = torch.empty(5, dtype=torch.int32, device=DEV)
    ms = torch.empty(5, device=DEV)
    mr = torch.empty(5, dtype=torch.int32, device=DEV)
    wsb = int(lib.fpm_mate_rank_ws_bytes(5))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    assert lib.fpm_mate_rank(*common, ptr(mc), ptr(ms), ptr(mr), ptr(ws), wsb, st) == 0
    _same((mc, ms, mr), ops.mate_rank(s, row, col, own))
    assert lib.fpm_mate_rank(*common, ptr(mc), ptr(ms), ptr(mr), ptr(ws), wsb - 8, st) != 0
    assert b"workspace" in lib.fpm_last_error()
    assert lib.fpm_mate_rank(ptr(s_d), 4499, 5, 4500, ptr(row_d), ptr(col_d), 0, P(0), ptr(mc), ptr(ms), ptr(mr),
                             ptr(ws), wsb, st) != 0
    assert b"mate_rank: bad sizes" in lib.fpm_last_error()

    edges = torch.linspace(-1.0, 1.0, 9)
    e_d = edges.to(DEV)
    gen = torch.full((10,), -1, dtype=torch.int64, device=DEV)
    imp, skipped = gen.clone(), gen[:3].clone()
    assert lib.fpm_score_census(*common, ptr(e_d), 9, ptr(gen), ptr(imp), ptr(skipped), st) == 0
    _same((gen, imp, skipped), ops.score_census(s, row, col, edges, own))
    for T in (0, 4096):
        assert lib.fpm_score_census(*common, ptr(e_d), T, ptr(gen), ptr(imp), ptr(skipped), st) != 0
        assert b"score_census: T" in lib.fpm_last_error()

    value, count = ctypes.c_float(), ctypes.c_long()
    wsb = int(lib.fpm_score_select_ws_bytes())
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    args = lambda cls, k, wsb_: common + (cls, k, ctypes.byref(value), ctypes.byref(count), ptr(ws), wsb_, st)
    assert lib.fpm_score_select(*args(2, 1000, wsb)) == 0
    hv, hn = ops.score_select(s, row, col, "impostor", 1000, own)
    assert count.value == hn and ctypes.c_int32.from_buffer_copy(value).value == int(_bits(hv.view(1))[0])
    assert lib.fpm_score_select(*args(2, 0, wsb)) != 0 and b"score_select: k" in lib.fpm_last_error()
    assert lib.fpm_score_select(*args(3, 1, wsb)) != 0 and b"score_select: cls" in lib.fpm_last_error()
    assert lib.fpm_score_select(*args(1, 1, wsb - 8)) != 0 and b"workspace" in lib.fpm_last_error()


# -------------------------------------------------------------------------------------- end to end
PROBE_LABELS = [1000, 1001, 1002]


def gallery_labels():
    """Each mated entry shares its probe's label; every other entry has a label of its own."""
    return [1000 + MATES[e] if e in MATES else e for e in range(40)]


@pytest.fixture(scope="module")
def labelled():
    gal, probes = planted()
    net = _net(state_dicts()["spread"])
    index = net.enroll(gal, DEV, batch=16, descriptors=True, subjects=gallery_labels())
    pset = net.enroll(probes, DEV, batch=2, descriptors=True, subjects=PROBE_LABELS)
    return net, pset, index


def _dense(index, plab):
    labels, col = torch.unique(index.subject, return_inverse=True)
    row = torch.tensor([labels.tolist().index(v) if v in labels.tolist() else -1 for v in plab], dtype=torch.int32)
    return row, col.to(torch.int32)


def test_stage_ranks_on_planted_gallery(labelled):
    net, pset, index = labelled
    sr = net.stage_ranks(pset, index)
    assert isinstance(sr, evaluate.StageRanks) and sr["stages"] == ["desc", "coarse", "coarse_subject"]
    mates = [e for p in range(3) for e, q in MATES.items() if q == p]
    for stage in ("desc", "coarse"):
        assert sr[stage]["mate_rank"].tolist() == [0, 0, 0], stage
        assert sr[stage]["mate_entry"].tolist() == mates and sr[stage]["mate_col"].tolist() == mates
        assert sr.recall(stage, 1) == 1.0 and sr.cmc(stage, (1, 5)) == [1.0, 1.0]
    assert sr["coarse_subject"]["mate_rank"].tolist() == [0, 0, 0]
    assert sr["coarse_subject"]["mate_subject"].tolist() == PROBE_LABELS
    # every figure equals ops.mate_rank of the host copy of the same matrix
    row, col = _dense(index, PROBE_LABELS)
    mats = dict(desc=ops.desc_score(pset.desc, index.desc).cpu(), coarse=net.coarse_scores_many(pset, index).cpu())
    for stage, m in mats.items():
        hc, hs, hr = ops.mate_rank(m, row, col)
        got = sr[stage]
        assert torch.equal(got["mate_col"], hc) and torch.equal(got["mate_rank"], hr), stage
        assert torch.equal(_bits(got["mate_score"]), _bits(hs)), stage
    # one probe a chunk, a selection, another route: the same ranks where the entries are the same
    again = evaluate.stage_ranks(net, pset, index, probe_chunk=1, coarse="any")
    for stage in sr["stages"]:
        assert torch.equal(again[stage]["mate_rank"], sr[stage]["mate_rank"]), stage
    part = net.stage_ranks(pset, index, select=[19, 3, 38, 5], probe_select=[2, 1])
    assert part["coarse"]["mate_entry"].tolist() == [38, 19] and part["coarse"]["mate_col"].tolist() == [2, 0]
    # probe 2 relabelled to an absent subject: non-mated at every stage
    pset.set_subjects([1000, 1001, 5555])
    try:
        sr2 = net.stage_ranks(pset, index)
    finally:
        pset.set_subjects(PROBE_LABELS)
    for stage in sr2["stages"]:
        assert sr2[stage]["mate_rank"].tolist() == [0, 0, -1] and sr2["mated"][stage].tolist() == [True, True, False]
        assert sr2.recall(stage, 1) == 1.0
    assert int(_bits(sr2["coarse"]["mate_score"])[2]) == QNAN


def test_stage_ranks_leave_one_out(labelled):
    net, pset, index = labelled
    labels = gallery_labels()
    labels[0] = labels[1] = 900                                   # entries 0 and 1: one subject
    index.set_subjects(labels)
    try:
        psel = [0, 1, 7]
        sr = net.stage_ranks(index, index, exclude_self=True, probe_select=psel)
        row, col = _dense(index, [900, 900, 1000])
        own = torch.tensor(psel, dtype=torch.int32)
        m = net.coarse_scores_many(index, index, probe_select=psel).cpu()
        hc, hs, hr = ops.mate_rank(m, row, col, own)
    finally:
        index.set_subjects(gallery_labels())
    got = sr["coarse"]
    assert torch.equal(got["mate_col"], hc) and torch.equal(got["mate_rank"], hr)
    assert torch.equal(_bits(got["mate_score"]), _bits(hs))
    assert got["mate_entry"].tolist() == [1, 0, -1] and int(hr[0]) >= 0 and int(hr[2]) == -1
    assert sr["coarse_subject"]["mate_rank"].tolist()[2] == -1    # entry 7 is its subject's only entry
    assert sr["coarse_subject"]["mate_subject"].tolist()[:2] == [900, 900]
    with pytest.raises(_lib.FpmError, match="probes is index"):
        net.stage_ranks(pset, index, exclude_self=True)
    with pytest.raises(_lib.FpmError, match="ShardedGallery"):
        net.stage_ranks(pset, ShardedGallery.split(index, [DEV, DEV]))


def test_search_report_on_planted_gallery(labelled):
    net, pset, index = labelled
    rep = net.evaluate_search(pset, index, ks=(1, 2), shortlist=4, prescreen=8, by=None, topk=4)
    assert rep["stages"]["prescreen"] == 1.0 and rep["stages"]["shortlist"] == 1.0
    assert rep["mated"] == 3 and rep["non_mated"] == 0 and "fnir" not in rep
    subject = index.subject
    # every per-probe flag from the identify_many result keys, on the host
    for q, (d, r) in enumerate(zip(rep["probes"], rep["results"])):
        mate = [e for e, p in MATES.items() if p == q][0]
        assert d["mated"] is True
        assert d["in_prescreen"] == (mate in r["pre_idx"].tolist())
        short = r["short_idx"].tolist()
        assert d["in_shortlist"] == (mate in short)
        sc = r["cls_prob"].view(-1).cpu().tolist()
        m = short.index(mate)
        above = sum(1 for j in range(len(short)) if j != m and (sc[j] > sc[m] or (sc[j] == sc[m] and j < m)))
        assert d["rank"] == above
        assert (d["rank"] == 0) == (int(r["top_idx"][0]) == mate)
    for k in (1, 2):
        assert rep["cmc"][k] == sum(d["rank"] < k for d in rep["probes"]) / 3
    # probe 2 non-mated; with a threshold every probe is decided
    pset.set_subjects([1000, 1001, 5555])
    try:
        rep = evaluate.search_report(net, pset, index, shortlist=4, threshold=-1.0)
    finally:
        pset.set_subjects(PROBE_LABELS)
    assert [d["mated"] for d in rep["probes"]] == [True, True, False] and rep["probes"][2]["rank"] == -1
    assert rep["probes"][0]["in_prescreen"] is None and rep["stages"]["prescreen"] is None
    match = [int(r["match"]) for r in rep["results"]]
    assert [d["match"] for d in rep["probes"]] == match
    assert rep["fpir"] == float(match[2] != -1)
    assert rep["fnir"] == sum(match[q] < 0 or int(subject[match[q]]) != PROBE_LABELS[q] for q in (0, 1)) / 2

"""Probe sets on the GPU: the pair-list instantiations of the three coarse kernels against their
one-probe siblings, the both-sides-cached batch (``match_pairs``) against the uncached forward,
``coarse_scores_many`` against the loop over probes, and ``identify_many`` (grouping, layouts,
de-duplication) against ``identify`` / ``run``.  Every comparison is bit for bit."""
import ctypes

import pytest
import torch

from fpm import _lib, gallery, ops, synth
from fpm.batch import DeviceBatch
from test_coarse_stream_cpu import STREAM_SHAPES
from test_coarse_wide_cpu import WIDE_SHAPES, synthetic_case
from test_compact_index_cpu import case
from test_compact_index_gpu import MIXED_N, MIXED_PROBES
from test_gallery_gpu import CASES
from test_shortlist_cpu import ENTRY_NS, PROBE_NS, SHAPES, coefficients, state_dicts
from test_shortlist_gpu import MATES, OUT_KEYS, _bits, _net, check_result_keys, planted

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
RUN_KEYS = ("s", "ss", "ds_mat", "perm_mat", "k_prob", "cls_prob")
ONE_PROBE = {"fused": ops.coarse_score, "wide": ops.coarse_score_wide, "stream": ops.coarse_score_stream}


@pytest.fixture(scope="module")
def sds():
    return state_dicts()


def _offsets(ns):
    return torch.tensor([0] + [sum(ns[:i + 1]) for i in range(len(ns))], dtype=torch.int64)


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).contiguous()


class _Store:
    """An entry row store and a probe row store on the device, with the host copies the ops take."""

    def __init__(self, y, row_off, yq, qrow_off, rows16=False):
        self.y = ops.cast_bf16(y.to(DEV)) if rows16 else y.to(DEV)
        self.row_off, self.yq, self.qrow_off = row_off, yq.to(DEV), qrow_off
        self.off_d, self.qoff_d = row_off.to(DEV), qrow_off.to(DEV)

    def pairs(self, kernel, q, g, coef, out=None):
        q, g = _i32(q), _i32(g)
        if out is None:
            out = torch.full((int(q.numel()),), float("nan"), device=DEV)
        return ops.coarse_pairs(self.y, self.off_d, g.to(DEV), self.yq, self.qoff_d, q.to(DEV), coef.to(DEV).contiguous(),
                                kernel=kernel, out=out, gidx_host=g, qidx_host=q, row_off_host=self.row_off,
                                qrow_off_host=self.qrow_off)

    def one_probe(self, kernel, q, g, coef):
        """The one-probe sibling over probe q's pairs."""
        g = _i32(g)
        yp = self.yq[int(self.qrow_off[q]):int(self.qrow_off[q + 1])]
        out = torch.full((int(g.numel()),), float("nan"), device=DEV)
        return ONE_PROBE[kernel](self.y, self.off_d, g.to(DEV), yp, coef.to(DEV).contiguous(), out=out, idx_host=g,
                                 row_off_host=self.row_off)


# ------------------------------------------------------- 1. pair-list kernel = its one-probe sibling
def _kernel_case(kernel):
    """The kernel's own shape set -> (y, row_off, [(n0, yp, idx, coef)], shapes, entry sizes)."""
    if kernel == "fused":
        sd, y, row_off, wg, probes = case()                      # ``ragged_case``, computed once per process
        idx = torch.tensor(list(range(len(ENTRY_NS))) + [2], dtype=torch.int32)
        out = [(n0, yp, idx, coefficients(wp, [wg[i] for i in idx.tolist()], sd))
               for (yp, wp), n0 in zip(probes, PROBE_NS)]
        return y, row_off, out, SHAPES, ENTRY_NS
    shapes = WIDE_SHAPES if kernel == "wide" else STREAM_SHAPES
    y, row_off, probes = synthetic_case("spread", shapes)
    return y, row_off, probes, shapes, sorted({b for _, b in shapes})


@pytest.mark.parametrize("rows", ["fp32", "bf16"])
@pytest.mark.parametrize("kernel", ["fused", "wide", "stream"])
def test_pair_list_kernel_equals_one_probe_kernel(kernel, rows):
    y, row_off, probes, shapes, entry_ns = _kernel_case(kernel)
    st = _Store(y, row_off, torch.cat([p[1] for p in probes]), _offsets([p[0] for p in probes]), rows16=rows == "bf16")
    assert st.y.dtype == (torch.bfloat16 if rows == "bf16" else torch.float32)
    q, g, pos, coefs, refs, seen = [], [], [], [], [], set()
    for k, (n0, yp, idx, coef) in enumerate(probes):
        refs.append(st.one_probe(kernel, k, idx, coef))
        q += [k] * idx.numel()
        g += idx.tolist()
        pos += list(range(idx.numel()))
        coefs.append(coef)
        seen |= {(n0, entry_ns[e]) for e in idx.tolist()}
    assert set(shapes) <= seen
    q, g, coef, ref = torch.tensor(q), torch.tensor(g), torch.cat(coefs), torch.cat(refs)
    assert bool(torch.isfinite(ref).all())
    # the pairs of different probes interleaved: neighbouring workgroups differ in n0 and in transposition
    inter = torch.argsort(torch.tensor(pos) * len(probes) + q, stable=True)
    assert len(set(q[inter][:len(probes)].tolist())) == len(probes)
    perm = torch.randperm(q.numel(), generator=torch.Generator().manual_seed(11))
    for order in (inter, perm):
        got = st.pairs(kernel, q[order], g[order], coef[order])
        assert torch.equal(_bits(got), _bits(ref[order.to(DEV)])), (kernel, rows)
    # one (probe, entry) pair named twice in a launch
    twice = torch.cat([inter, inter[3:4]])
    got = st.pairs(kernel, q[twice], g[twice], coef[twice])
    assert torch.equal(_bits(got), _bits(ref[twice.to(DEV)])) and int(_bits(got)[3]) == int(_bits(got)[-1])


# ------------------------------------------------------------------------------- 2. persistent walk
@pytest.mark.parametrize("kernel", ["wide", "stream"])
def test_persistent_walk_over_the_grid(kernel):
    """300 pairs on the 256-workgroup grid, small boxes: a workgroup walks pairs of different probes."""
    gen = torch.Generator().manual_seed(77)
    pn, en, B = (5, 33, 40), (2, 17, 48), 300
    st = _Store(torch.randn(sum(en), 768, generator=gen) * 0.22, _offsets(en),
                torch.randn(sum(pn), 768, generator=gen) * 0.22, _offsets(pn))
    b = torch.arange(B)
    q, g = b % 3, (b // 3 + b // 7) % 3
    coef = torch.tanh(torch.randn(B, 768, generator=gen))
    assert len(set(zip(q.tolist(), g.tolist()))) == 9 and len({(int(q[i]), int(q[i + 256])) for i in range(44)}) > 1
    got = st.pairs(kernel, q, g, coef)
    assert bool(torch.isfinite(got).all())
    for k in range(3):
        m = q == k
        assert torch.equal(_bits(got[m.to(DEV)]), _bits(st.one_probe(kernel, k, g[m], coef[m]))), (kernel, k)


# ---------------------------------------------------------------------------------- 3. stream slots
def test_stream_slots_from_the_largest_probe_and_the_largest_entry():
    """Pairs (600, 1) and (1, 600) in one launch: the largest probe and the largest entry are of
    different pairs."""
    gen = torch.Generator().manual_seed(78)
    st = _Store(torch.randn(601, 768, generator=gen) * 0.22, _offsets((1, 600)),
                torch.randn(601, 768, generator=gen) * 0.22, _offsets((600, 1)))
    coef = torch.tanh(torch.randn(2, 768, generator=gen))
    got = st.pairs("stream", [0, 1], [0, 1], coef)
    assert bool(torch.isfinite(got).all())
    for k in range(2):
        assert torch.equal(_bits(got[k:k + 1]), _bits(st.one_probe("stream", k, [k], coef[k:k + 1])))


# --------------------------------------------------------------- 4. match_pairs = the uncached forward
PAIR_PROBE_N = {"f32ops-f32": (48, 40, 44), "f32ops-bf16": (48, 40, 44), "bf16ops": (72, 60, 66)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_match_pairs_equals_uncached(name, sds):
    dtype, _, ns, sc_mode = CASES[name]
    gal = [synth.make_graph(40, p, 1, n) for p, n in enumerate(ns)]
    prb = [synth.make_graph(41, p, 0, n) for p, n in enumerate(PAIR_PROBE_N[name])]
    net = _net(sds["flat"], dtype)
    index = net.enroll(gal, DEV, sc_mode=sc_mode, batch=4)
    pset = net.enroll(prb, DEV, sc_mode=sc_mode, batch=2)
    G = len(gal)
    # ragged, repeated probes and entries, one pair twice, not probe-major
    pairs = [(2, G - 1), (0, 0), (1, 3), (2, 1), (0, G - 1), (1, 3), (0, 2)]
    ref = net.run(DeviceBatch.from_pairs([(prb[q], gal[g]) for q, g in pairs], DEV), chunks=2)
    res = net.match_pairs(pset, index, pairs, chunks=2)
    for k in RUN_KEYS:
        assert res[k].dtype == ref[k].dtype and torch.equal(res[k], ref[k]), (name, k)
    assert set(ref) <= set(res)
    with pytest.raises(_lib.FpmError, match="a probe number outside"):
        net.match_pairs(pset, index, [(3, 0)])
    with pytest.raises(_lib.FpmError, match="an entry number outside"):
        net.match_pairs(pset, index, [(0, G)])


# ---------------------------------------------------------------------- the planted-mate gallery
@pytest.fixture(scope="module")
def mates(sds):
    gal, probes = planted()
    net = _net(sds["spread"])
    idx = {lay: net.enroll(gal, DEV, batch=16, layout=lay) for lay in ("f32", "f32+bf16", "bf16+host")}
    return net, probes, gal, idx, net.enroll(probes, DEV, batch=2)


# ------------------------------------------------------------- 5. coarse_scores_many = the loop
def test_coarse_scores_many_equals_the_loop(mates, monkeypatch):
    net, probes, gal, idx, pset = mates
    index = idx["f32"]
    loop = net.coarse_scores(probes, index)
    many = net.coarse_scores_many(pset, index)
    assert many.dtype == torch.float32 and many.device == index.device and tuple(many.shape) == (3, len(gal))
    assert bool(torch.isfinite(many).all()) and torch.equal(_bits(many), _bits(loop))
    for p in range(len(probes)):
        assert int(many[p].argmax()) == [e for e, q in MATES.items() if q == p][0]
    sel = torch.randperm(len(gal), generator=torch.Generator().manual_seed(5))[:23]
    psel = [2, 0]
    loop_s = net.coarse_scores([probes[p] for p in psel], index, select=sel)
    assert torch.equal(_bits(net.coarse_scores_many(pset, index, probe_select=psel, select=sel)), _bits(loop_s))
    # several launches walked: 7 pairs each
    monkeypatch.setattr(gallery, "COARSE_PAIRS_CHUNK", 7)
    assert torch.equal(_bits(net.coarse_scores_many(pset, index)), _bits(loop))
    assert torch.equal(_bits(net.coarse_scores_many(pset, index, probe_select=psel, select=sel)), _bits(loop_s))


# ------------------------------------------------------------------------------ 6. mixed routes
def test_coarse_scores_many_mixed_routes(sds):
    gal = [synth.make_graph(42, p, 1, n) for p, n in enumerate(MIXED_N)]
    probes = [synth.make_graph(42, p, 0, n) for p, n in enumerate(MIXED_PROBES)]
    net = _net(sds["spread"])
    index = net.enroll(gal, DEV, batch=4)
    pset = net.enroll(probes, DEV, batch=2)
    # all three kernels in one launch's worth of pairs; per probe the sets of the one-probe pass
    nq = pset.n.long().repeat_interleave(index.G)
    assert sorted(set(gallery.coarse_routes(nq, index.n.long().repeat(pset.G), "any").tolist())) == [0, 1, 2]
    assert [sorted(set(gallery.coarse_routes(n0, index.n, "any").tolist())) for n0 in MIXED_PROBES] \
        == [[0, 1, 2], [1, 2], [2]]
    loop = net.coarse_scores(probes, index, coarse="any")
    many = net.coarse_scores_many(pset, index, coarse="any")
    assert bool(torch.isfinite(many).all()) and torch.equal(_bits(many), _bits(loop))
    with pytest.raises(_lib.FpmError, match="COARSE_WIDE_NMAX"):
        net.coarse_scores_many(pset, index, coarse="auto")


# ------------------------------------------------------------------------------- 7. identify_many
def _group_pairs_of(res, order):
    """(probe, entry) pairs of each group, rebuilt from the per-probe dicts."""
    groups = {}
    for p in order:
        gi, b0, b1 = res[p]["group"]
        groups.setdefault(gi, []).append((b0, b1, p))
    return {gi: sorted(v) for gi, v in groups.items()}


def test_identify_many_groups(mates):
    net, probes, gal, idx, pset = mates
    index = idx["f32"]
    res = net.identify_many(pset, index, topk=5, shortlist=8, group_pairs=16)
    one = net.identify(probes, index, topk=5, shortlist=8)
    assert len(res) == len(probes)
    for a, b in zip(res, one):
        check_result_keys(a, "identify_many", None, True, k=5, M=8, Gs=len(gal))
        check_result_keys(b, "identify", None, True, k=5, M=8, Gs=len(gal))
        assert torch.equal(_bits(a["coarse_all"]), _bits(b["coarse_all"]))
        assert a["short_idx"].dtype == torch.int32 and torch.equal(a["short_idx"], b["short_idx"])
        assert torch.equal(_bits(a["coarse_score"]), _bits(b["coarse_score"]))
    # probes of 48, 33 and 40 keypoints, 8 pairs each, 16 per group: [33, 40] then [48], yet the
    # results come back in the caller's order
    assert [r["group"] for r in res] == [(1, 0, 8), (0, 0, 8), (0, 8, 16)]
    assert gallery.probe_groups(pset.n, 8, 16) == [[1, 2], [0]]
    for gi, members in _group_pairs_of(res, range(len(probes))).items():
        pairs = [(p, int(e)) for _, _, p in members for e in res[p]["short_idx"].tolist()]
        ref = net.run(DeviceBatch.from_pairs([(probes[q], gal[g]) for q, g in pairs], DEV))
        for b0, b1, p in members:
            for k in RUN_KEYS:
                assert torch.equal(res[p][k], ref[k][b0:b1]), (gi, p, k)
    for r in res:
        hi, hs = ops.rank_topk(r["cls_prob"].cpu().view(1, -1), 5)
        assert torch.equal(r["top_idx"].cpu(), r["short_idx"].cpu()[hi[0].long()])
        assert torch.equal(_bits(r["top_score"].cpu()), _bits(hs[0]))
    # without a shortlist every probe meets every selected entry, in selection order
    sel = [5, 2, 7, 30]
    full = net.identify_many(pset, index, topk=2, select=sel, probe_select=[2, 1])
    ref = net.match_pairs(pset, index, [(q, g) for q in (1, 2) for g in sel])        # groups sort by n: 33 then 40
    for r, b0 in zip(full, (4, 0)):
        check_result_keys(r, "identify_many", None, False, k=2)
        assert "short_idx" not in r and r["group"] == (0, b0, b0 + 4)
        for k in RUN_KEYS:
            assert torch.equal(r[k], ref[k][b0:b0 + 4]), k
        assert set(r["top_idx"].tolist()) <= set(sel)


# --------------------------------------------------------------------------------- 8. uniform box
def test_identify_many_uniform_box_equals_identify(sds):
    dtype, _, ns, sc_mode = CASES["f32ops-f32"]
    gal = [synth.make_graph(40, p, 1, n) for p, n in enumerate(ns)]
    prb = [synth.make_graph(41, p, 0, 48) for p in range(3)]
    net = _net(sds["flat"], dtype)
    index = net.enroll(gal, DEV, sc_mode=sc_mode, batch=4)
    pset = net.enroll(prb, DEV, sc_mode=sc_mode, batch=2)
    G = len(gal)
    res = net.identify_many(pset, index, topk=3, shortlist=G)
    assert [r["group"][0] for r in res] == [0, 0, 0]            # one group: every query's box is (48, 48)
    for p, r in enumerate(res):
        ref = net.identify(prb[p], index, topk=3, shortlist=G)
        for k in OUT_KEYS + ("short_idx",):
            assert r[k].dtype == ref[k].dtype and torch.equal(r[k], ref[k]), (p, k)


# ------------------------------------------------------------------------------------- 9. layouts
def test_identify_many_layouts_agree(mates, monkeypatch):
    net, probes, gal, idx, pset = mates
    ref = net.identify_many(pset, idx["f32"], topk=5, shortlist=8, group_pairs=16)
    for lay in ("f32+bf16", "bf16+host"):
        res = net.identify_many(pset, idx[lay], topk=5, shortlist=8, group_pairs=16)
        for a, b in zip(res, ref):
            assert a["group"] == b["group"]
            for k in OUT_KEYS + ("short_idx",):
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (lay, k)
            for k in ("coarse_score", "coarse_all"):
                assert torch.equal(_bits(a[k]), _bits(b[k])), (lay, k)
    # the distinct entries of a batch over the staging cap are refused, with fetch's message
    monkeypatch.setattr(gallery, "FETCH_MAX_BYTES", 2 * 3072)
    with pytest.raises(_lib.FpmError, match="shortlist="):
        net.match_pairs(pset, idx["bf16+host"], [(0, 1), (1, 2)])
    with pytest.raises(_lib.FpmError, match="probe set's layout"):
        net.identify_many(idx["bf16+host"], idx["f32"], shortlist=2)


# ----------------------------------------------------------------------------- 10. de-duplication
def test_identify_many_exclude_self(mates):
    net, probes, gal, idx, pset = mates
    index = idx["f32"]
    G = len(gal)
    res = net.identify_many(index, index, shortlist=3, topk=3, exclude_self=True)
    assert len(res) == G
    call = torch.stack([r["coarse_all"] for r in res]).cpu()
    masked = call.clone()
    masked[torch.arange(G), torch.arange(G)] = float("-inf")
    hi, hs = ops.rank_select(masked, 3)
    for q, r in enumerate(res):
        assert q not in r["short_idx"].tolist()
        assert torch.equal(r["short_idx"].cpu(), hi[q]) and torch.equal(_bits(r["coarse_score"].cpu()), _bits(hs[q]))
        assert q not in r["top_idx"].tolist() and tuple(r["cls_prob"].shape) == (3,)
    plain = net.identify_many(index, index, shortlist=3, topk=3)
    assert [int(r["short_idx"][0]) for r in plain] == list(range(G))      # without the flag q ranks itself first
    for a, b in zip(plain, res):
        assert torch.equal(_bits(a["coarse_all"]), _bits(b["coarse_all"]))
    # the shortlist is clamped to len(select) - 1; without a shortlist the self pair is left out
    few = net.identify_many(index, index, shortlist=64, select=[4, 9, 6], probe_select=[9, 4], exclude_self=True)
    assert [sorted(r["short_idx"].tolist()) for r in few] == [[4, 6], [6, 9]]
    few = net.identify_many(index, index, select=[4, 9, 6], probe_select=[9, 4], exclude_self=True)
    assert [sorted(r["top_idx"].tolist()) for r in few] == [[4, 6], [6, 9]]
    with pytest.raises(_lib.FpmError, match="exclude_self"):
        net.identify_many(pset, index, shortlist=3, exclude_self=True)


# ------------------------------------------------------------------------------------- 11. C ABI
def test_pair_list_c_abi_entry_points():
    gen = torch.Generator().manual_seed(79)
    pn, en = (40, 129, 257, 601), (24, 48)
    y, yq = torch.randn(sum(en), 768, generator=gen) * 0.22, torch.randn(sum(pn), 768, generator=gen) * 0.22
    st, st16 = _Store(y, _offsets(en), yq, _offsets(pn)), _Store(y, _offsets(en), yq, _offsets(pn), rows16=True)
    lib = _lib.load()
    P = ctypes.c_void_p
    stream = P(torch.cuda.current_stream(DEV).cuda_stream)
    B, G, Q = 4, len(en), len(pn)
    q, g = _i32([0, 0, 0, 0]).to(DEV), _i32([0, 1, 1, 0]).to(DEV)
    coef = torch.tanh(torch.randn(B, 768, generator=gen)).to(DEV)
    wsb = max(int(lib.fpm_coarse_score_wide_ws_bytes(B)), int(lib.fpm_coarse_score_stream_ws_bytes(B, 601, 48)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    cases = [("fused", lib.fpm_coarse_pairs, lib.fpm_coarse_pairs_rows16, (), b"COARSE_NMAX"),
             ("wide", lib.fpm_coarse_pairs_wide, lib.fpm_coarse_pairs_wide_rows16, (P(ws.data_ptr()), wsb),
              b"COARSE_WIDE_NMAX"),
             ("stream", lib.fpm_coarse_pairs_stream, lib.fpm_coarse_pairs_stream_rows16, (P(ws.data_ptr()), wsb),
              b"COARSE_STREAM_NMAX")]
    for k, (kernel, fn32, fn16, wsa, bound) in enumerate(cases):
        for fn, s in ((fn32, st), (fn16, st16)):
            args = lambda qi, out: (P(s.y.data_ptr()), P(s.off_d.data_ptr()), P(g.data_ptr()), G, B, P(s.yq.data_ptr()),
                                    P(s.qoff_d.data_ptr()), P(qi.data_ptr()), Q, P(coef.data_ptr()), 10, 0.01,
                                    P(out.data_ptr())) + wsa + (stream,)
            got = torch.full((B,), float("nan"), device=DEV)
            assert fn(*args(q, got)) == 0
            ref = s.pairs(kernel, q.cpu(), g.cpu(), coef)
            assert bool(torch.isfinite(got).all()) and torch.equal(_bits(got), _bits(ref)), kernel
            # a probe over the kernel's bound: refused by name, nothing launched
            over = _i32([0, k + 1, 0, 0]).to(DEV)
            untouched = torch.full((B,), float("nan"), device=DEV)
            rc = fn(*args(over, untouched))
            assert rc != 0 and bound in lib.fpm_last_error(), (kernel, lib.fpm_last_error())
            a = list(args(q, untouched))
            a[5] = P(0)
            rc = fn(*a)
            assert rc != 0 and b"are required" in lib.fpm_last_error()
            torch.cuda.synchronize()
            assert bool(torch.isnan(untouched).all())

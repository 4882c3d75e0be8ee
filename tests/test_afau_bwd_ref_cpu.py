"""The float64 stage references of the AFA-U backward (tests/afau_bwd_ref.py) held to what the project
already trusts: chained the way afau_grad.backward chains the kernels, they reproduce torch.autograd
through fpm.afau_torch.afau_ks (pinned to the oracle by tests/test_train_cpu.py) for every regressor
parameter.  Also the tie rule of the max-pool seed and the one-hot input mode."""
import functools

import torch

from fpm import afau_torch, params
import afau_bwd_ref as R

ZERO_GRAD = ("Wq.weight", "Wk.weight", "col_encoding_block.Wv.weight", "col_encoding_block.mixed_score_MHA.mix1_weight",
             "col_encoding_block.mixed_score_MHA.mix1_bias", "col_encoding_block.mixed_score_MHA.mix2_weight",
             "col_encoding_block.mixed_score_MHA.mix2_bias", "col_encoding_block.multi_head_combine.weight",
             "multi_head_combine.bias", "mixed_score_MHA.mix2_bias",
             # a per-channel constant in front of an instance norm is cancelled by it, like the combine biases
             "feed_forward.W2.bias")


def _group(k):
    """The chain tests' scale groups (tests/test_train.py): per head, per encoder block."""
    return k.split(".")[0] + ("." + k.split(".")[3] if k.startswith("encoder_k") else "")


@functools.lru_cache(maxsize=None)
def _case():
    sd = params.init_params(6)
    g = torch.Generator().manual_seed(2)
    n1, n2 = (12, 9, 12), (10, 12, 10)                    # ragged, n2 = 10 twice: Bu < B
    ss = torch.zeros(3, 12, 12, dtype=torch.float64)
    for b in range(3):
        ss[b, :n1[b], :n2[b]] = torch.softmax(torch.randn(n1[b], n2[b], generator=g, dtype=torch.float64) * 3, dim=1)
    names = [k for k in sd if k.startswith(afau_torch.AFAU_PARAM_PREFIXES) and sd[k].is_floating_point()]
    dks = torch.tensor([0.3, -1.0, 0.7], dtype=torch.float64)
    leaves = {k: sd[k].double().clone().requires_grad_(True) for k in names}
    ks = afau_torch.afau_ks(ss, torch.tensor(n1), torch.tensor(n2), lambda k: leaves[k])
    (ks * dks).sum().backward()
    auto = {k: leaves[k].grad for k in names}
    got = R.chain(ss, n1, n2, lambda k: sd[k], dks, names, torch.float64)
    return names, auto, got


def test_chain_equals_autograd():
    names, auto, got = _case()
    scale = {}
    for k in names:
        if auto[k] is not None:
            scale[_group(k)] = max(scale.get(_group(k), 0.0), float(auto[k].abs().max()))
    checked = 0
    for k in names:
        ref = auto[k] if auto[k] is not None else torch.zeros_like(got[k])
        s = scale[_group(k)]
        assert s > 0, k
        row_mix1 = k.endswith("row_encoding_block.mixed_score_MHA.mix1_weight")
        if row_mix1 or k.endswith(ZERO_GRAD):
            # analytically zero (all of the tensor; of the row block's mix1_weight, row 0, which
            # multiplies the zero dot product): 0, or at most 1e-12 of the group's scale
            for t in (got[k], ref):
                z = t[:, 0] if row_mix1 else t
                assert float(z.abs().max()) <= 1e-12 * s, k
            if not row_mix1:
                continue
        err = float((got[k] - ref).abs().max())
        assert err <= 1e-10 * float(ref.abs().max()), (k, err, float(ref.abs().max()))
        checked += 1
    assert checked >= 20


def test_every_parameter_covered():
    names, auto, got = _case()
    assert set(got) == set(names)
    # the parameters the chain leaves at zero are exactly the analytically-zero ones
    for k in names:
        if float(got[k].abs().max()) == 0.0:
            assert k.endswith(ZERO_GRAD), k


def test_maxpool_seed_tie_rule():
    """Two exactly equal maxima: the seed goes to the smaller position, all of it."""
    B, P, Cn = 2, 37, 5
    g = torch.Generator().manual_seed(3)
    y = torch.randn(B, P, Cn, generator=g, dtype=torch.float64)
    y[:, 20, :] = 9.0
    y[:, 3, :] = 9.0
    assert torch.equal(R.pool_argmax(y), torch.full((B, Cn), 3))
    assert torch.equal(R.pool_argmax(y, tie="last"), torch.full((B, Cn), 20))
    # through the norm: x with two equal entries above the rest keeps them equal in y
    x = torch.randn(B, P, Cn, generator=g)
    x[:, 20, :] = 5.0
    x[:, 3, :] = 5.0
    w, b = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g)
    gs = torch.randn(B, Cn, generator=g)
    yy = R.instnorm_fwd(x, w, b)
    assert torch.equal(yy[:, 3], yy[:, 20]) and torch.equal(R.pool_argmax(yy), torch.full((B, Cn), 3))
    _, dw, db = R.instnorm_bwd(x, w, b, gseed=gs)
    assert (db - gs.double()).abs().max() < 1e-15                 # the whole seed, once
    xh = (yy - b.double()) / w.double()
    assert (dw - gs.double() * xh[:, 3]).abs().max() < 1e-12
    dx1, _, _ = R.instnorm_bwd(x, w, b, gseed=gs)
    dx2, _, _ = R.instnorm_bwd(x, w, b, gseed=gs, tie="last")
    assert (dx1[:, 3] - dx2[:, 20]).abs().max() < 1e-12 and (dx1[:, 3] - dx1[:, 20]).abs().min() > 1e-6


def test_onehot_mode_equals_explicit_input():
    B, P, Cn = 3, 12, 20
    g = torch.Generator().manual_seed(4)
    bias = torch.randn(Cn, generator=g) * 0.1
    nvalid = [12, 5, 0]
    x = R.onehot_input(B, P, Cn, nvalid, bias)
    ex = torch.zeros(B, P, Cn, dtype=torch.float64)
    for b, nv in enumerate(nvalid):
        for p in range(nv):
            ex[b, p, p] = 1.0
    ex += bias.double()
    assert torch.equal(x, ex)
    w, bb = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g)
    dy = torch.randn(B, P, Cn, generator=g)
    dx, dw, db = R.instnorm_bwd(x, w, bb, dy=dy)
    # constant channels (c >= nvalid): xhat = 0, so dw = 0 and dx = 0 up to float64 rounding of the mean
    for b, nv in enumerate(nvalid):
        assert dw[b, nv:].abs().max() < 1e-10
    assert (db - dy.double().sum(1)).abs().max() < 1e-12


def test_glue():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(7, 3, 5, generator=g)
    key = torch.tensor([0, 2, 0, 2, 2, 0, 0])
    out = R.rows_sum(x, key=key, nkeys=3)
    assert torch.equal(out[1], torch.zeros(3, 5, dtype=torch.float64))
    assert (out.sum(0) - R.rows_sum(x)).abs().max() < 1e-12
    t = R.transpose_pad(x[:, 0], 8)
    assert t.shape == (5, 8) and torch.equal(t[:, :7], x[:, 0].t()) and (t[:, 7:] == 0).all()
    assert torch.equal(R.relu_mask(x, x), torch.relu(x)) and torch.equal(R.add(x, x), 2 * x)
    assert (R.wgrad(x[:, 0], x[:, 1]) - torch.einsum("ri,rj->ij", x[:, 0].double(), x[:, 1].double())).abs().max() < 1e-12


# ------------------------------------------------------------------------------------------ mutation check
def _gate(ref, ref32):
    """The device tests' rule: max(2^-20 max|ref|, 8 max|ref32 - ref|) of one output tensor."""
    return max(2.0 ** -20 * float(ref.abs().max()), 8.0 * float((ref32.double() - ref).abs().max()))


def test_mutations_move_the_reference_past_the_gate():
    """The gates of tests/test_afau_bwd_stages.py can see the errors they exist for: each mistake below,
    applied to the float64 reference's input at the device tests' own cases, moves the reference by
    more than the gate the device is held to.  (The module is imported for its case builders only; its
    tests need a GPU, these lines do not.)"""
    import test_afau_bwd_stages as S
    # one masked column: j < n2 becoming j <= n2, at every case with a pair whose n2 < n2max
    seen = 0
    for si, variant in S.ATTN_CASES:
        B, n1max, n2max, n2s = S.ATTN_SHAPES[si]
        if variant == "ref" or all(v == n2max for v in n2s):
            continue
        for wkind in ("init", "edge"):
            cost, datt, ref, ref32, _ = S._attn_case(si, variant, wkind)
            w = [S._weights(wkind)[k] for k in S.ATTN_KEYS]
            mut = R.attn_bwd(cost, [min(v + 1, n2max) for v in n2s], *w, datt, torch.float64)
            assert float((mut[0] - ref[0]).abs().max()) > _gate(ref[0], ref32[0]), (si, variant, wkind)
            seen += 1
    assert seen >= 6
    # one dropped position (the last), at every instance-norm case with more than one position
    seen = 0
    for B, P, Cn in S.NORM_SHAPES:
        if P == 1:
            continue
        w, b, cases = S._norm_cases(B, P, Cn)
        for cs in cases:
            dy, gs = cs["call"].get("dy"), cs["call"].get("gseed")
            ref = R.instnorm_bwd(cs["x64"], w, b, dy=dy, gseed=gs)
            ref32 = R.instnorm_bwd(cs["x32"], w, b, dy=dy, gseed=gs, dtype=torch.float32)
            mut = R.instnorm_bwd(cs["x64"][:, :P - 1], w, b, dy=None if dy is None else dy[:, :P - 1], gseed=gs)
            moved = [float((mut[0] - ref[0][:, :P - 1]).abs().max()) > _gate(ref[0], ref32[0]),
                     float((mut[1] - ref[1]).abs().max()) > _gate(ref[1], ref32[1])]
            assert any(moved), (B, P, Cn, cs["tag"])
            seen += 1
    assert seen == 7 * 7
    # the tie rule flipped
    for B, P, Cn, tie in S.TIE_CASES:
        w, b, x1, x2, gs = S._tie_case(B, P, Cn, tie)
        x64 = x1.double() + x2.double()
        ref = R.instnorm_bwd(x64, w, b, gseed=gs)
        ref32 = R.instnorm_bwd(x1 + x2, w, b, gseed=gs, dtype=torch.float32)
        mut = R.instnorm_bwd(x64, w, b, gseed=gs, tie="last")
        assert float((mut[0] - ref[0]).abs().max()) > _gate(ref[0], ref32[0])

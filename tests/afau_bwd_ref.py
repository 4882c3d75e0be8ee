"""Float64 references of the AFA-U backward, stage by stage (csrc/afau_bwd.hip, fpm/afau_grad.py).
Plain torch on the CPU: every vector-Jacobian product is autograd over a direct statement of the
stage, written from fpm/afau_torch.py and the kernels' comments.  No kernels, no library calls.  Test
helper only -- shared by test_afau_bwd_ref_cpu.py (which holds the chained stages to autograd through
fpm.afau_torch.afau_ks) and test_afau_bwd_stages.py (which holds the kernels to the stages).

Every function takes ``dtype``: float64 gives the reference, float32 the "ref32" figure of the
project's tolerance rule (tests/test_afau_stages.py).  Per-pair partials are obtained by giving
every pair its own copy of the parameters as autograd leaves.

Layouts, as the kernels':
  head part (B, 2 * (8 E + 17)):  [dW0 (8 x E) | db0 (8) | dw2 (8) | db2] of the row head, then the
                                  same of the column head
  attention mix_part (B, 16, 49): [dW2 (16) | dW1 row 1 (16) | db1 (16) | db2]
  attention dwv_part (B, 256, n2max)
"""
import math

import torch
import torch.nn.functional as F

from fpm import config as C

E, H, D, MS = C.AFAU_EMB, C.AFAU_HEADS, C.AFAU_QKV, C.AFAU_MS_HIDDEN
PRE = "encoder_k.layers.0."
HEAD_KEYS = ("final_row.0.weight", "final_row.0.bias", "final_row.2.weight", "final_row.2.bias",
             "final_col.0.weight", "final_col.0.bias", "final_col.2.weight", "final_col.2.bias")


def _leaf(t, dtype, B=None):
    """A fresh autograd leaf of ``t`` in ``dtype``; with ``B``: one copy per pair, (B, *t.shape)."""
    t = t.detach().to(dtype)
    if B is not None:
        t = t.unsqueeze(0).expand(B, *t.shape)
    return t.clone().requires_grad_(True)


# ------------------------------------------------------------------------------------------ heads
def head_hidden(gr, gc, hp, dtype=torch.float64):
    """Hidden pre-activations (B, 2, 8) of final_row(gr) and final_col(gc) (the ReLU's branch input)."""
    p = lambda k: hp[k].to(dtype)
    return torch.stack((F.linear(gr.to(dtype), p("final_row.0.weight"), p("final_row.0.bias")),
                        F.linear(gc.to(dtype), p("final_col.0.weight"), p("final_col.0.bias"))), dim=1)


def head_bwd(gr, gc, hp, dks, dtype=torch.float64):
    """ks = sigmoid((final_row(gr) + final_col(gc)) / 2), seeded with dks -> (dgr, dgc, part)."""
    B, En = gr.shape
    g = [_leaf(gr, dtype), _leaf(gc, dtype)]
    k = []
    leaves = []
    for q, head in enumerate(("final_row", "final_col")):
        W0, b0 = _leaf(hp[head + ".0.weight"], dtype, B), _leaf(hp[head + ".0.bias"], dtype, B)
        w2 = _leaf(hp[head + ".2.weight"].reshape(8), dtype, B)
        b2 = _leaf(hp[head + ".2.bias"].reshape(1), dtype, B)
        hid = torch.einsum("bme,be->bm", W0, g[q]) + b0
        k.append((torch.relu(hid) * w2).sum(1) + b2[:, 0])
        leaves += [W0, b0, w2, b2]
    ks = torch.sigmoid((k[0] + k[1]) / 2)
    (ks * dks.to(dtype)).sum().backward()
    part = torch.cat([t.grad.reshape(B, -1) for t in leaves], dim=1)
    assert part.shape == (B, 2 * (8 * En + 17))
    return g[0].grad, g[1].grad, part


# ------------------------------------------------------------------------------------------ instance norm
def onehot_input(B, P, Cn, nvalid, bias, dtype=torch.float64):
    """The column block's synthesised input: onehot(p == c and p < nvalid[b]) + bias[c], (B, P, Cn)."""
    p = torch.arange(P)[None, :, None]
    c = torch.arange(Cn)[None, None, :]
    nv = torch.as_tensor(nvalid).view(B, 1, 1)
    return ((p == c) & (p < nv)).to(dtype) + bias.to(dtype)[None, None, :]


def _xhat(x, eps):
    """InstanceNorm1d over positions without the affine part; x (B, P, Cn)."""
    if x.shape[1] == 1:
        # F.instance_norm refuses a single position; its statistics are mean = x and variance 0
        return (x - x) / math.sqrt(eps)
    return F.instance_norm(x.transpose(1, 2), eps=eps).transpose(1, 2)


def instnorm_fwd(x, w, b, dtype=torch.float64, eps=C.IN_EPS):
    """y = instnorm_over_positions(x) * w + b; x (B, P, Cn)."""
    return _xhat(x.to(dtype), eps) * w.to(dtype) + b.to(dtype)


def pool_argmax(y, tie="first"):
    """Position (B, Cn) of the max over positions of y (B, P, Cn); ties go to the smallest position
    (``tie="last"``: to the largest -- the flipped rule of the mutation check)."""
    is_max = (y == y.max(dim=1, keepdim=True).values).to(torch.int32)
    if tie == "first":
        return is_max.argmax(dim=1)
    assert tie == "last"
    return y.shape[1] - 1 - is_max.flip(1).argmax(dim=1)


def instnorm_bwd(x, w, b, dy=None, gseed=None, dtype=torch.float64, eps=C.IN_EPS, tie="first"):
    """y = instnorm_over_positions(x) * w + b with x (B, P, Cn) (in1, in1 + in2 or onehot_input(...),
    formed by the caller in ``dtype``'s precision from the fp32 operands).  Seed: dense dy (B, P, Cn),
    or gseed (B, Cn) routed through max over positions of y -> (dx, dw_part (B, Cn), db_part (B, Cn))."""
    assert (dy is None) != (gseed is None)
    B = x.shape[0]
    xl, wl, bl = _leaf(x, dtype), _leaf(w, dtype, B), _leaf(b, dtype, B)
    y = _xhat(xl, eps) * wl[:, None, :] + bl[:, None, :]
    if gseed is not None:
        pm = pool_argmax(y.detach(), tie)
        loss = (y.gather(1, pm[:, None, :])[:, 0, :] * gseed.to(dtype)).sum()
    else:
        loss = (y * dy.to(dtype)).sum()
    loss.backward()
    return xl.grad, wl.grad, bl.grad


# ------------------------------------------------------------------------------------------ attention
def attn_pre(cost, w1, b1, dtype=torch.float64):
    """Hidden pre-activations c w1_h + b1_h of the mixed score, (B, H, R, Cn, MS), R0 = 0 (the
    dot-product input is 0, so only row 1 of mix1_weight acts)."""
    c = cost.to(dtype)
    return c[:, None, :, :, None] * w1.to(dtype)[None, :, 1, None, None, :] + b1.to(dtype)[None, :, None, None, :]


def attn_fwd(cost, n2, Wv, w1, b1, w2, b2, dtype=torch.float64):
    """-> (out (B * R, 256), stats (B * R, 16, 2) = softmax (max, sum of exp(score - max)))."""
    B, R, Cn = cost.shape
    pre = attn_pre(cost, w1, b1, dtype)
    score = (torch.relu(pre) * w2.to(dtype).reshape(1, H, 1, 1, MS)).sum(-1) + b2.to(dtype).reshape(1, H, 1, 1)
    mask = (torch.arange(Cn)[None, :] < torch.as_tensor(n2).view(B, 1)).to(dtype)
    v = Wv.to(dtype)[:, :Cn].reshape(1, H, D, Cn) * mask[:, None, None, :]
    M = score.max(dim=3).values
    ex = torch.exp(score - M[..., None])
    S = ex.sum(3)
    out = torch.einsum("bhrj,bhdj->brhd", ex / S[..., None], v).reshape(B * R, H * D)
    return out, torch.stack((M, S), dim=-1).permute(0, 2, 1, 3).reshape(B * R, H, 2)


def attn_bwd(cost, n2, Wv, w1, b1, w2, b2, datt, dtype=torch.float64):
    """The row block's cross-set attention with R0 = 0: out_h(i) = sum_j softmax_j(f_h(cost_ij)) v_h(j),
    f_h(c) = relu(c w1_h + b1_h) . w2_h + b2_h, v_h(j) = Wv[h*16:(h+1)*16, j] for j < n2[b], 0 beyond;
    every row i < n1max is a real row.  datt (B * R, 256) -> (dwv_part (B, 256, Cn), mix_part (B, 16, 49))."""
    B, R, Cn = cost.shape
    c = cost.to(dtype)
    Wl = _leaf(Wv[:, :Cn], dtype, B)                                   # (B, 256, Cn)
    w1l, b1l = _leaf(w1[:, 1, :], dtype, B), _leaf(b1, dtype, B)         # (B, H, MS)
    w2l, b2l = _leaf(w2.reshape(H, MS), dtype, B), _leaf(b2.reshape(H), dtype, B)
    pre = c[:, None, :, :, None] * w1l[:, :, None, None, :] + b1l[:, :, None, None, :]
    score = (torch.relu(pre) * w2l[:, :, None, None, :]).sum(-1) + b2l[:, :, None, None]
    att = torch.softmax(score, dim=3)                                   # (B, H, R, Cn)
    mask = (torch.arange(Cn)[None, :] < torch.as_tensor(n2).view(B, 1)).to(dtype)
    v = Wl.reshape(B, H, D, Cn) * mask[:, None, None, :]
    out = torch.einsum("bhrj,bhdj->brhd", att, v).reshape(B * R, H * D)
    (out * datt.to(dtype)).sum().backward()
    mix = torch.cat((w2l.grad, w1l.grad, b1l.grad, b2l.grad[:, :, None]), dim=2)
    return Wl.grad, mix


# ------------------------------------------------------------------------------------------ glue
def rows_sum(x, key=None, nkeys=1, dtype=torch.float64):
    """Sum over the leading dim; with ``key``: out[u] = sum of x[b] with key[b] == u."""
    x = x.to(dtype)
    if key is None:
        return x.sum(0)
    out = torch.zeros(nkeys, *x.shape[1:], dtype=dtype)
    return out.index_add_(0, torch.as_tensor(key).long(), x)


def transpose_pad(x, ldo):
    """(R, C) -> (C, ldo) with zero columns beyond R."""
    return F.pad(x.t(), (0, ldo - x.shape[0]))


def wgrad(dY, X, dtype=torch.float64):
    """dY^T X (N1 x N2) for dY (R x N1), X (R x N2)."""
    return dY.to(dtype).t() @ X.to(dtype)


def relu_mask(x, ref):
    """ReLU backward through the post-activation: x where ref > 0, else 0."""
    return torch.where(ref > 0, x, torch.zeros_like(x))


def add(x, ref):
    return x + ref


# ------------------------------------------------------------------------------------------ the chain
def chain(ss, n1, n2, P, dks, names, dtype=torch.float64):
    """The stages above chained the way afau_grad.forward / backward chain the kernels: parameter
    gradients (dict by name; analytically-zero ones as zeros) of sum(ks * dks).  ``P(name)`` returns
    a parameter (reference state_dict names)."""
    B, n1max, n2max = ss.shape
    g = lambda blk, k: P(PRE + blk + "_encoding_block." + k).detach().to(dtype)
    ssd = ss.to(dtype)
    n2l = [int(v) for v in n2]
    n2u, inv = torch.unique(torch.tensor(n2l), return_inverse=True)
    Bu = int(n2u.numel())
    mixw = [g("row", "mixed_score_MHA." + k) for k in ("mix1_weight", "mix1_bias", "mix2_weight", "mix2_bias")]
    att, _ = attn_fwd(ssd, n2l, g("row", "Wv.weight"), *mixw, dtype=dtype)
    mh = F.linear(att, g("row", "multi_head_combine.weight"), g("row", "multi_head_combine.bias"))
    sv = {}
    for blk, nb, Pn in (("row", B, n1max), ("col", Bu, n2max)):
        x1 = mh.view(B, n1max, E) if blk == "row" else onehot_input(
            Bu, n2max, E, n2u, g(blk, "multi_head_combine.bias"), dtype)
        o1 = instnorm_fwd(x1, g(blk, "add_n_normalization_1.norm.weight"), g(blk, "add_n_normalization_1.norm.bias"),
                          dtype)
        h = torch.relu(F.linear(o1, g(blk, "feed_forward.W1.weight"), g(blk, "feed_forward.W1.bias")))
        ff = F.linear(h, g(blk, "feed_forward.W2.weight"), g(blk, "feed_forward.W2.bias"))
        y2 = instnorm_fwd(o1 + ff, g(blk, "add_n_normalization_2.norm.weight"),
                          g(blk, "add_n_normalization_2.norm.bias"), dtype)
        sv[blk] = dict(x1=x1, o1=o1, h=h, ff=ff, gm=y2.max(dim=1).values, nb=nb, P=Pn)
    gr, gc = sv["row"]["gm"], sv["col"]["gm"][inv]
    hp = {k: P(k).detach() for k in HEAD_KEYS}
    grads = {}
    dgr, dgc, part = head_bwd(gr, gc, hp, dks, dtype)
    hs = rows_sum(part, dtype=dtype)
    PS = 8 * E + 17
    for q, head in enumerate(("final_row", "final_col")):
        o = q * PS
        grads[head + ".0.weight"] = hs[o:o + 8 * E].view(8, E)
        grads[head + ".0.bias"] = hs[o + 8 * E:o + 8 * E + 8]
        grads[head + ".2.weight"] = hs[o + 8 * E + 8:o + 8 * E + 16].view(1, 8)
        grads[head + ".2.bias"] = hs[o + 8 * E + 16:o + 8 * E + 17]
    dgcu = rows_sum(dgc, key=inv, nkeys=Bu, dtype=dtype)
    for blk, seed in (("row", dgr), ("col", dgcu)):
        st = sv[blk]
        rows = st["nb"] * st["P"]
        pre = PRE + blk + "_encoding_block."
        dx2, dwp, dbp = instnorm_bwd(st["o1"] + st["ff"], g(blk, "add_n_normalization_2.norm.weight"),
                                     g(blk, "add_n_normalization_2.norm.bias"), gseed=seed, dtype=dtype)
        grads[pre + "add_n_normalization_2.norm.weight"] = rows_sum(dwp, dtype=dtype)
        grads[pre + "add_n_normalization_2.norm.bias"] = rows_sum(dbp, dtype=dtype)
        dx2 = dx2.reshape(rows, E)
        h, o1 = st["h"].reshape(rows, -1), st["o1"].reshape(rows, E)
        dpre = relu_mask(dx2 @ g(blk, "feed_forward.W2.weight"), h)
        grads[pre + "feed_forward.W2.weight"] = wgrad(dx2, h, dtype)
        grads[pre + "feed_forward.W2.bias"] = rows_sum(dx2, dtype=dtype)
        grads[pre + "feed_forward.W1.weight"] = wgrad(dpre, o1, dtype)
        grads[pre + "feed_forward.W1.bias"] = rows_sum(dpre, dtype=dtype)
        do1 = add(dpre @ g(blk, "feed_forward.W1.weight"), dx2)
        dmh, dwp, dbp = instnorm_bwd(st["x1"], g(blk, "add_n_normalization_1.norm.weight"),
                                     g(blk, "add_n_normalization_1.norm.bias"),
                                     dy=do1.view(st["nb"], st["P"], E), dtype=dtype)
        grads[pre + "add_n_normalization_1.norm.weight"] = rows_sum(dwp, dtype=dtype)
        grads[pre + "add_n_normalization_1.norm.bias"] = rows_sum(dbp, dtype=dtype)
        if blk == "col":
            continue
        dmh = dmh.reshape(rows, E)
        grads[pre + "multi_head_combine.weight"] = wgrad(dmh, att, dtype)
        grads[pre + "multi_head_combine.bias"] = rows_sum(dmh, dtype=dtype)
        datt = dmh @ g(blk, "multi_head_combine.weight")
        dwvp, mixp = attn_bwd(ssd, n2l, g(blk, "Wv.weight"), *mixw, datt, dtype=dtype)
        dwv = torch.zeros(H * D, E, dtype=dtype)
        dwv[:, :n2max] = rows_sum(dwvp, dtype=dtype)
        grads[pre + "Wv.weight"] = dwv
        mix = rows_sum(mixp, dtype=dtype)
        m1 = torch.zeros(H, 2, MS, dtype=dtype)
        m1[:, 1] = mix[:, 16:32]
        grads[pre + "mixed_score_MHA.mix1_weight"] = m1
        grads[pre + "mixed_score_MHA.mix1_bias"] = mix[:, 32:48]
        grads[pre + "mixed_score_MHA.mix2_weight"] = mix[:, 0:16].reshape(H, MS, 1)
        grads[pre + "mixed_score_MHA.mix2_bias"] = mix[:, 48:49]
    return {k: grads[k].reshape(P(k).shape) if k in grads else torch.zeros(P(k).shape, dtype=dtype) for k in names}

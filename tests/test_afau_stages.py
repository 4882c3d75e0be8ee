"""The AFA-U k regressor's fp32 / bf16 forward kernels (csrc/afau.hip, Net._afau), stage by stage
against the float64 oracle: the row-block cross-set attention, the instance norm, the 600 -> 8 -> 1
heads, and the whole chain.

Tolerance rule (every stage): ``ref`` is the oracle in float64 on the fp32 inputs the kernel sees,
``ref32`` the same oracle function in float32 on the CPU, ``err32 = max|ref32 - ref|``.  The device
must stay within ``max(floor, 8 * err32)``; the floors are the project's kernel-agreement bounds
(test_crossset_attn_lds_v_kernel, test_crossset_attn_split_rows, test_afau_gemm_norm_*).  A fixed
bound would not do: with the model's own init (mix weights U(-10, 10)) the scores reach ~1e3 and the
CPU fp32 attention already sits ~3e-5 x max|ref| from float64, with weights of scale 2 ~1e-6.  The
factor 8 covers a max over ~1e5 outputs under another summation order plus fast_exp2; one wrong LUT
segment or one mis-masked column moves an output by >= 1e-3 x max|ref|.

Which attention case reaches which instantiation of fpm_crossset_attn_fwd (every one in fp32 output
= 16-term scores, bf16 output and split output; "v" is set_tuning("afau_attn_v", v)):

  kernel                       scores (bf16 / split)   cases (n2max)
  afau_row_attn_v_kernel<16>   FAST interval form      45, 64, 256 at v = 1
  afau_row_attn_v_kernel<32>   FAST interval form      257, 512 at v = 1
  afau_row_attn_kernel<16>     LUT (use_lut = 1)       45, 64, 256 at v = 0
  afau_row_attn_kernel<40>     LUT (use_lut = 1)       257, 512 at v = 0; 513, 600 (production path)

MEASURED: the largest device_err / err32 per stage and output type over all cases of a run on an
MI355X (attention: per kernel; "lse" = M + log(sum) of the softmax stats; bf16 outputs: the error
left after the 2^-8 x max|ref| rounding allowance is not separable, so the figure is the fraction of
the gate used).  The gates do not use these numbers.
"""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpm
from fpm import _lib, ops, params
import oracle as O
from oracle import ngm_oracle as NO

from test_gpu_parity import BF16_MEASURED

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROW = "encoder_k.layers.0.row_encoding_block"
MIX = ROW + ".mixed_score_MHA."
NB = 64                       # score-LUT buckets over [0, 1] (AF_NB in csrc/afau.hip)

MEASURED = {
    # attention, device_err / err32 ("ldsv" = afau_row_attn_v_kernel, "gather" = afau_row_attn_kernel)
    "attn.ldsv.f32": 1.26, "attn.gather.f32": 1.34,
    # split rows: the largest ratio is an "edge" case (err32 = 7e-8 absolute), where the error left
    # is the hi + lo representation itself, 2^-17 relative per value; 0.30 of the gate (its floor)
    "attn.ldsv.split": 7.26, "attn.gather.split": 7.26,
    # bf16 rows: fraction of the gate (2^-9 x max|ref| of it is the store's own rounding)
    "attn.ldsv.bf16": 0.80, "attn.gather.bf16": 0.80,
    "attn.ldsv.lse": 1.91, "attn.gather.lse": 1.74,
    # instance norm.  Before the kernel kept its values relative to the channel's first position
    # this was 12.8 (one-hot mode, P = 257; 10.3 at P = 256): the constant channels c >= nvalid came
    # out as rstd = 316 times the rounding error of their fp32 mean
    "instnorm.out_f": 3.73, "instnorm.gmax": 3.73,
    "head": 1.0,
    # whole chain: max |ks - ks64| (gates 1e-4, 1e-4, 1.74e-3, 1.74e-3)
    "chain.f32": 1.3e-7, "chain.bf16x3": 2.5e-7, "chain.bf16s": 1.2e-4, "chain.bf16": 1.3e-4,
}


def _i32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32, device=DEV)


def _report(tag, err, err32, gate):
    """One figure line per check, printed before the assertion (collected with ``pytest -s``)."""
    print("MEASURE %s err=%.3g err32=%.3g ratio=%.3g gate=%.3g frac=%.3g"
          % (tag, err, err32, err / err32 if err32 > 0 else float("inf") if err > 0 else 0.0, gate, err / gate))


def _gate_check(tag, dev, ref, ref32, floor, extra=0.0):
    """The common rule.  ``floor``: a number or a tensor shaped like ``ref`` (elementwise floor);
    ``extra``: an allowance added to the gate (the bf16 store's rounding)."""
    ref = ref.double()
    err32 = float((ref32.double() - ref).abs().max())
    d = (dev.double() - ref).abs()
    assert torch.isfinite(dev).all(), tag
    gate = torch.clamp(torch.as_tensor(floor, dtype=torch.float64), min=8.0 * err32) + extra
    worst = float((d / gate).max())
    _report(tag, float(d.max()), err32, float(gate.max()))
    assert worst <= 1.0, "%s: device error %.3g over the gate (err32 %.3g, %.2f x gate)" % (
        tag, float(d.max()), err32, worst)


@functools.lru_cache(maxsize=None)
def _sd():
    return params.init_params(7)


# ------------------------------------------------------------------------------------- attention
def _breakpoints(wsd):
    """The kernel's fp32 breakpoints t = -b1 / w1 of every head's hidden units (inf where w1 = 0)."""
    w1 = wsd[MIX + "mix1_weight"][:, 1, :]
    b1 = wsd[MIX + "mix1_bias"]
    return torch.where(w1 != 0, -b1 / w1, torch.full_like(w1, float("inf")))


@functools.lru_cache(maxsize=None)
def _weights(kind):
    """"init": init_params(7) (mix weights U(-10, 10)).  "edge": mix weights U(-2, 2), Wv as at init,
    heads 0-4 constructed (see the checks at the end)."""
    sd = _sd()
    if kind == "init":
        return sd
    sd = dict(sd)
    g = torch.Generator().manual_seed(101)
    u = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1) * 2
    w1a, b1a, w2a, b2a = u(16, 2, 16), u(16, 16), u(16, 16, 1), u(16, 1)
    m = torch.arange(16, dtype=torch.float32)
    sgn = torch.where(m % 2 == 0, 1.0, -1.0)                # units active above / below their breakpoint

    def place(h, w1, t):
        w1a[h, 1] = w1
        b1a[h] = -w1 * t
    # head 0: all 16 breakpoints inside bucket [10/64, 11/64): 5+ in one bucket -> 16-term fallback
    place(0, sgn * (1 + 0.125 * m), (10 + (m + 1) / 18) / 64)
    # head 1: breakpoints exactly at the bucket edges 4m / 64 (powers of two: -b1 / w1 is exact)
    place(1, sgn * 2, 4 * m / 64)
    # head 2: w1 = 0 on every other unit, both signs of b1 among them
    w1a[2, 1, 1::2] = 0
    b1a[2, 1::2] = torch.tensor([1.5, -0.75, 0.5, -1.25, 1.0, -0.5, 0.25, -1.75])
    # head 3: breakpoints exactly at 0, 0.5 and 1
    place(3, sgn * 4, torch.tensor([0.0, 0.5, 1.0]).repeat(6)[:16])
    # head 4: every breakpoint outside [0, 1]
    place(4, sgn * 1.5, torch.where(m < 8, -0.5 - 0.25 * m, 1.5 + 0.25 * (m - 8)))
    sd[MIX + "mix1_weight"], sd[MIX + "mix1_bias"] = w1a, b1a
    sd[MIX + "mix2_weight"], sd[MIX + "mix2_bias"] = w2a, b2a
    t = _breakpoints(sd)
    assert ((t[0] >= 10 / 64) & (t[0] < 11 / 64)).all()
    assert torch.equal(t[1], 4 * m / 64)
    assert torch.isinf(t[2, 1::2]).all() and (b1a[2, 1::2] > 0).any() and (b1a[2, 1::2] < 0).any()
    assert set(t[3].tolist()) == {0.0, 0.5, 1.0}
    assert ((t[4] < 0) | (t[4] > 1)).all()
    return sd


def _costs(B, n1max, n2max, n2s, wsd, oob, seed):
    """rand^4 in fp32, exact zeros past each pair's n2 (at least the row's last 3 columns), and in
    pair 0 (n2 = n2max): an exact 1.0, k / 64 for k < 8, six values in bucket 10, three breakpoints
    of the weights, 0.5 and 12 / 64; ``oob``: -0.25 and 1.5 (the kernel's out-of-range fallback)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(B, n1max, n2max, generator=g) ** 4
    for b in range(B):
        c[b, :, min(n2s[b], n2max - 3):] = 0
    c[0, 0, 0] = 1.0
    c[0, 1, :8] = torch.arange(8, dtype=torch.float32) / 64
    c[0, 2, :6] = (10 + torch.tensor([0.0, 0.11, 0.37, 0.52, 0.78, 0.96])) / 64
    t = _breakpoints(wsd)
    inside = t[(t > 0) & (t < 1)]
    c[0, 3, 0], c[0, 3, 1] = inside[0], inside[-1]
    if 0 < float(t[0, 3]) < 1:
        c[0, 3, 2] = t[0, 3]
    c[0, 3, 3], c[0, 3, 4] = 0.5, 12 / 64
    if oob:
        c[0, 4, 0], c[0, 4, 1] = -0.25, 1.5
    return c


def _landing_checks(wsd, cost, edge):
    """From the weights and costs alone: the inputs reach the score paths they are meant for."""
    t = _breakpoints(wsd)                                               # (16 heads, 16 units)
    edges = torch.arange(NB + 1, dtype=torch.float32) / NB
    cnt = ((t[:, :, None] >= edges[None, None, :-1]) & (t[:, :, None] < edges[None, None, 1:])).sum(1)   # (16, NB)
    cin = cost[(cost >= 0) & (cost <= 1)]
    bk = torch.clamp((cin * NB).long(), max=NB - 1)
    hit = torch.zeros(NB, dtype=torch.bool)
    hit[bk] = True
    assert (((cnt >= 1) & (cnt <= 4)) & hit[None, :]).any(), "no cost in a bucket with 1-4 breakpoints"
    assert torch.isin(cost, t[torch.isfinite(t)]).any(), "no cost equal to a breakpoint"
    assert (cost == 1.0).any() and (cost == 0.0).any()
    if edge:
        assert cnt[0, 10] >= 5 and hit[10], "head 0 / bucket 10: the 16-term fallback is not reached"
        assert cnt[1, 4] == 1 and (cost == 4 / 64).any()                 # a cost on a bucket-edge breakpoint


def _attn_oracle(wsd, cost, n2s, dtype):
    """oracle.afau_attention on the reference's inputs R0 = 0, C0 = one-hot (ngm.py:392-399) ->
    (pre-combine output (B * R, 256), logsumexp of the mixed scores (B * R, 16))."""
    B, R, Cn = cost.shape
    a = torch.zeros(B, R, 600, dtype=dtype)
    bemb = torch.zeros(B, Cn, 600, dtype=dtype)
    for b in range(B):
        bemb[b, torch.arange(n2s[b]), torch.arange(n2s[b])] = 1.0
    mixed, out = O.afau_attention(a, bemb, cost.to(dtype), wsd, ROW)
    return out.reshape(B * R, 256), torch.logsumexp(mixed, dim=3).permute(0, 2, 1).reshape(B * R, 16)


ATTN_SHAPES = [
    (3, 37, 45, [45, 20, 1]),       # last row tile 5 rows, n2 = 1, load_v scalar tail, unaligned cost rows
    (2, 16, 64, [64, 61]),          # float4 cost path
    (2, 33, 256, [256, 255]),       # TJ = 16 limit
    (1, 17, 257, [257]),            # first TJ = 32 shape
    (2, 20, 512, [512, 437]),       # LDS-V limit
    (1, 18, 513, [513]),            # gather kernel TJ = 40; bf16 modes: the production LUT path
    (1, 16, 600, [600]),            # the reference's largest box
]
ATTN_CASES = [(i, "plain") for i in range(len(ATTN_SHAPES))] + [(0, "oob"), (1, "view")]


@pytest.mark.parametrize("wkind", ["init", "edge"])
@pytest.mark.parametrize("si,variant", ATTN_CASES, ids=["%d-%s" % (ATTN_SHAPES[i][2], v) for i, v in ATTN_CASES])
def test_crossset_attn_vs_f64(si, variant, wkind):
    """ops.crossset_attn (fp32, bf16 and split outputs, softmax stats; both kernels where both apply)
    against oracle.afau_attention in float64.  "oob": two costs outside [0, 1]; "view": the cost is a
    row-strided view of a wider buffer."""
    B, n1max, n2max, n2s = ATTN_SHAPES[si]
    wsd = _weights(wkind)
    cost = _costs(B, n1max, n2max, n2s, wsd, variant == "oob", 1000 * si + n1max)
    _landing_checks(wsd, cost, wkind == "edge")
    ref, lse = _attn_oracle(wsd, cost, n2s, torch.float64)
    ref32, lse32 = _attn_oracle(wsd, cost, n2s, torch.float32)
    scale = float(ref.abs().max())
    lse_floor = 1e-5 * torch.clamp(lse.abs(), min=1.0)
    if variant == "view":
        buf = torch.full((B, n1max, n2max + 4), 0.5, device=DEV)
        cost_d = buf[:, :, :n2max]
        cost_d.copy_(cost)
        assert not cost_d.is_contiguous()
    else:
        cost_d = cost.to(DEV)
    n2_d = _i32(n2s)
    w = [wsd[k].to(DEV).contiguous() for k in (ROW + ".Wv.weight", MIX + "mix1_weight", MIX + "mix1_bias",
                                                MIX + "mix2_weight", MIX + "mix2_bias")]
    rows = B * n1max
    for v in ((1, 0) if n2max <= 512 else (None,)):
        kern = "ldsv" if v == 1 else "gather"
        pv = ops.set_tuning("afau_attn_v", v) if v is not None else None
        try:
            got = {}
            for kind in ("f32", "bf16", "split"):
                out = torch.full((rows, 768 if kind == "split" else 256), float("nan"), device=DEV,
                                 dtype=torch.float32 if kind == "f32" else torch.bfloat16)
                st = torch.full((rows, 16, 2), float("nan"), device=DEV)
                ops.crossset_attn(cost_d, n2_d, *w, out, split=kind == "split", stats=st)
                torch.cuda.synchronize()
                got[kind] = (out.cpu(), st.cpu())
        finally:
            if pv is not None:
                ops.set_tuning("afau_attn_v", pv)
        for kind, (out, st) in got.items():
            tag = "attn.%s.%s" % (kern, kind)
            if kind == "split":
                assert torch.equal(out[:, 512:], out[:, :256])
                val = out[:, :256].float() + out[:, 256:512].float()
            else:
                val = out.float()
            floor = {"f32": 1e-5, "bf16": 1e-5, "split": 2e-5}[kind] * scale
            _gate_check(tag, val, ref, ref32, floor, extra=2.0 ** -8 * scale if kind == "bf16" else 0.0)
            assert (st[..., 1] > 0).all()
            _gate_check("attn.%s.lse.%s" % (kern, kind), st[..., 0].double() + st[..., 1].double().log(), lse, lse32,
                        lse_floor)


def test_crossset_attn_rejects_strided_columns():
    """The kernels read cost rows with a unit inner stride: any other view is refused on the host."""
    wsd = _weights("init")
    w = [wsd[k].to(DEV).contiguous() for k in (ROW + ".Wv.weight", MIX + "mix1_weight", MIX + "mix1_bias",
                                                MIX + "mix2_weight", MIX + "mix2_bias")]
    cost = torch.rand(2, 45, 16, device=DEV).transpose(1, 2)            # (2, 16, 45), inner stride 16
    out = torch.empty(2 * 16, 256, device=DEV)
    with pytest.raises(_lib.FpmError):
        ops.crossset_attn(cost, _i32([45, 45]), *w, out)
    wide = torch.rand(2, 16, 90, device=DEV)[:, :, ::2]                 # every other column
    with pytest.raises(_lib.FpmError):
        ops.crossset_attn(wide, _i32([45, 45]), *w, out)


# ------------------------------------------------------------------------------------- instance norm
def _bf16_ulp(x):
    """Spacing of bfloat16 (8 significant bits) at |x|."""
    _, e = torch.frexp(x.abs().clamp(min=2.0 ** -120))
    return torch.ldexp(torch.ones_like(x), e - 8)


def _norm_input(kind, B, P, Cn, g):
    """"normal": unit normal; "offset": per-channel offsets of +-50 with unit spread; "const": unit
    normal with one constant channel.  The constant is dyadic (0.75 * P is exact in fp32 in any
    summation order): with a value whose mean rounds, the output of a zero-variance channel is
    rstd = 316 times the mean's rounding error -- summation-order noise of any fp32 evaluation, the
    CPU's included, not a property of the kernel."""
    x = torch.randn(B, P, Cn, generator=g)
    if kind == "offset":
        x = x + 50.0 * torch.where(torch.arange(Cn) % 2 == 0, 1.0, -1.0)
    elif kind == "const":
        x[:, :, 3] = 0.75
    return x


@pytest.mark.parametrize("B,P,Cn", [(3, 1, 600), (2, 16, 600), (3, 37, 600), (2, 256, 600), (2, 257, 600),
                                    (1, 600, 600), (2, 40, 70)])
def test_instnorm_vs_f64(B, P, Cn):
    """ops.instnorm (NV = 16 up to 256 positions, NV = 40 beyond; P = 1: variance 0; Cn = 70: a
    partial 64-channel block) against oracle._instnorm in float64: in1, in1 + in2 and the one-hot
    column-block mode (C0 + bias synthesised in the kernel, nvalid ones on the diagonal), each as
    fp32 rows, fp32 rows + the zero-K-padded bf16 copy (ldt = 640), and the fused max over positions."""
    g = torch.Generator().manual_seed(1000 * P + Cn)
    w = torch.rand(Cn, generator=g) + 0.5
    b = torch.randn(Cn, generator=g) * 0.1
    w_d, b_d = w.to(DEV), b.to(DEV)
    LDT = 640
    cases = []
    for kind in ("normal", "offset", "const"):
        x1 = _norm_input(kind, B, P, Cn, g)
        x2 = torch.randn(B, P, Cn, generator=g)
        if kind == "const":
            x2[:, :, 3] = 0.5
        cases.append((kind + ".in1", x1, dict(in1=x1.to(DEV))))
        cases.append((kind + ".in1+in2", x1 + x2, dict(in1=x1.to(DEV), in2=x2.to(DEV))))
    bias = torch.randn(Cn, generator=g) * 0.1
    nvalid = [P, 1, P // 2][:B]
    c0 = torch.zeros(B, P, Cn)
    for i, nv in enumerate(nvalid):
        d = torch.arange(min(nv, P, Cn))
        c0[i, d, d] = 1.0
    cases.append(("onehot", c0 + bias, dict(in1=None, nvalid=_i32(nvalid), onehot_bias=bias.to(DEV))))
    for name, x, kw in cases:
        ref = NO._instnorm(x.double(), w.double(), b.double())
        ref32 = NO._instnorm(x, w, b)
        in1 = kw.pop("in1")
        of = torch.full((B * P, Cn), float("nan"), device=DEV)
        ops.instnorm(in1, B, P, Cn, w_d, b_d, out_f=of, **kw)
        of2 = torch.full((B * P, Cn), float("nan"), device=DEV)
        ot = torch.full((B * P, LDT), 7.0, device=DEV, dtype=torch.bfloat16)
        ops.instnorm(in1, B, P, Cn, w_d, b_d, out_f=of2, out_t=ot, ldt=LDT, **kw)
        gm = torch.full((B, Cn), float("nan"), device=DEV)
        ops.instnorm(in1, B, P, Cn, w_d, b_d, gmax=gm, **kw)
        torch.cuda.synchronize()
        of, of2, ot, gm = of.cpu().view(B, P, Cn), of2.cpu().view(B, P, Cn), ot.cpu(), gm.cpu()
        _gate_check("instnorm.out_f", of, ref, ref32, 2e-5)
        _gate_check("instnorm.out_f", of2, ref, ref32, 2e-5)
        t = ot[:, :Cn].float().view(B, P, Cn)
        assert ((t - of2).abs() <= _bf16_ulp(of2)).all(), name
        assert (ot[:, Cn:] == 0).all(), name
        _gate_check("instnorm.gmax", gm, ref.max(dim=1).values, ref32.max(dim=1).values, 2e-5)


def test_instnorm_position_cap():
    """641 positions exceed the 40-values-per-thread instantiation: refused, nothing launched."""
    x = torch.zeros(641, 64, device=DEV)
    w = torch.ones(64, device=DEV)
    with pytest.raises(_lib.FpmError):
        ops.instnorm(x, 1, 641, 64, w, w, out_f=torch.empty(641, 64, device=DEV))


# ------------------------------------------------------------------------------------- heads
@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("B", [1, 5])
def test_afau_head_vs_f64(B, moved):
    """ops.afau_head against sigmoid((final_row(gr) + final_col(gc)) / 2) in float64 (ngm.py:406-412).
    ``moved``: two first-layer biases of the row head shifted by +-5, so that hidden units of both
    signs (ReLU active and inactive) occur for certain."""
    sd = dict(_sd())
    if moved:
        bb = sd["final_row.0.bias"].clone()
        bb[0] += 5.0
        bb[1] -= 5.0
        sd["final_row.0.bias"] = bb
    E = 600
    g = torch.Generator().manual_seed(40 + B)
    gr = torch.rand(B, E, generator=g) * 6 - 3
    gc = torch.rand(B, E, generator=g) * 6 - 3

    def head(dt):
        p = lambda k: sd[k].to(dt)
        hr = F.linear(gr.to(dt), p("final_row.0.weight"), p("final_row.0.bias"))
        hc = F.linear(gc.to(dt), p("final_col.0.weight"), p("final_col.0.bias"))
        kr = F.linear(F.relu(hr), p("final_row.2.weight"), p("final_row.2.bias")).squeeze(-1)
        kc = F.linear(F.relu(hc), p("final_col.2.weight"), p("final_col.2.bias")).squeeze(-1)
        return torch.sigmoid((kr + kc) / 2), hr
    ref, hid = head(torch.float64)
    ref32, _ = head(torch.float32)
    if moved:
        assert (hid > 0).any() and (hid < 0).any()
    d = lambda k: sd[k].to(DEV).reshape(-1).contiguous()
    ks = torch.full((B,), float("nan"), device=DEV)
    ops.afau_head(gr.to(DEV), gc.to(DEV), B, E, d("final_row.0.weight"), d("final_row.0.bias"),
                  d("final_row.2.weight"), d("final_row.2.bias"), d("final_col.0.weight"), d("final_col.0.bias"),
                  d("final_col.2.weight"), d("final_col.2.bias"), ks)
    torch.cuda.synchronize()
    _gate_check("head", ks.cpu(), ref, ref32, 1e-6)


# ------------------------------------------------------------------------------------- whole chain
def _tailview(n1, n2):
    n_host = [torch.tensor(n1, dtype=torch.int32), torch.tensor(n2, dtype=torch.int32)]
    return types.SimpleNamespace(B=len(n1), device=DEV, nmax=[max(n1), max(n2)], n=[t.to(DEV) for t in n_host],
                                 n_host=n_host, n1=n_host[0].to(DEV), n2=n_host[1].to(DEV), n1max=max(n1),
                                 n2max=max(n2))


@functools.lru_cache(maxsize=None)
def _ks_case(n1, n2):
    """(fp32 ss, float64 oracle ks on it): Sinkhorn outputs, zero outside each pair's block."""
    B, n1max, n2max = len(n1), max(n1), max(n2)
    g = torch.Generator().manual_seed(sum(n1))
    s = torch.randn(B, n1max, n2max, generator=g, dtype=torch.float64) * 0.02
    ss = O.pygm_sinkhorn(s, n1, n2, dummy_row=True, max_iter=10, tau=0.01).float()
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in _sd().items()}
    return ss, O.afau_ks(ss.double(), torch.tensor(n1), torch.tensor(n2), sd64)


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16s", "bf16"])
@pytest.mark.parametrize("n1,n2", [((128, 120, 97), (128, 128, 101)),      # fused norms, P = 128, last tile half empty
                                   ((40, 33), (37, 40)),                   # unfused
                                   ((72,), (301,))],                       # TJ = 32 attention, NV = 40 column norm
                         ids=["128", "40", "72x301"])
def test_afau_chain_vs_f64(n1, n2, mode):
    """Net._afau (attention -> combine -> norms / FFN -> max -> heads, the column block per distinct
    n2) in every AFA-U operand mode against oracle.afau_ks in float64 on the same fp32 ss."""
    ss, ref = _ks_case(n1, n2)
    net = fpm.Net(regression=True, backbone=False, dtype="f32" if mode == "f32" else "bf16",
                  afau=None if mode == "f32" else mode)
    net.load_state_dict(_sd())
    assert net.afau_mode == mode
    ks = net._afau(net.packed(DEV), ss.to(DEV), _tailview(list(n1), list(n2)))
    torch.cuda.synchronize()
    err = float((ks.cpu().double() - ref).abs().max())
    gate = 1e-4 if mode in ("f32", "bf16x3") else 2.0 * BF16_MEASURED["k_prob"]
    print("MEASURE chain.%s err=%.3g gate=%.3g frac=%.3g" % (mode, err, gate, err / gate))
    assert err < gate

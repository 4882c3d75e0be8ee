"""The AFA-U backward kernels (csrc/afau_bwd.hip, driven by fpm/afau_grad.py) stage by stage against
the float64 references of tests/afau_bwd_ref.py, then the whole backward at the sizes that reach the
forms the 160-row test in test_train.py does not.

Tolerance rule (every stage; the project's own, tests/test_afau_stages.py): ``ref`` is the float64
reference on exactly the fp32 inputs the kernel sees, ``ref32`` the same function in float32 on the
CPU, ``err32 = max|ref32 - ref|`` per output tensor.  The device must be finite and within
``max(floor, 8 * err32)`` with ``floor = 2^-20 * max|ref|`` (16 ulp of the tensor's scale; it only
matters where err32 happens to be 0).  Outputs that are exactly determined are compared for equality:
the max pool's seed landing on one position (db_part == gseed), zero regions, mp[48], the sums of
dyadic values.

Branch decisions are fixed by the inputs, never by leaving anything out: the head's hidden units keep
|hid| >= 1e-3 max|hid|, the max-pool seed's top-2 gap is >= 1e-3 of the channel's spread, no mixed-score
pre-activation lies within 2^-20 (|c w1| + |b1|) of its kink unless it is exactly 0 in fp32 with an
exact product (then the kernel's ``pre > 0`` and torch's ReLU backward both give 0).  Each margin is
asserted on the CPU side before the kernel runs.

Which case reaches which entry point and instantiation:

  entry point / form                       cases
  fpm_afau_head_bwd                        test_head_bwd[B = 1, 5; moved, dead]
  instnorm_bwd_kernel<16>                  test_instnorm_bwd[P = 1, 16, 37, 256, 40x70]
  instnorm_bwd_kernel<40>                  test_instnorm_bwd[P = 257, 600, 640]
  partial 64-channel tile                  test_instnorm_bwd[(2, 40, 70)] (Cn = 70), [(1, 600, 600)] (600 = 9 x 64 + 24)
  instnorm accumulate = 1, dx = null       test_instnorm_bwd_accumulate, test_instnorm_bwd_no_dx
  afau_attn_bwd_kernel<1>                  test_attn_bwd[45, 256]
  afau_attn_bwd_kernel<2>                  test_attn_bwd[257, 512]
  afau_attn_bwd_kernel<3>                  test_attn_bwd[513, 600]
  fpm_rows_sum one level / two levels      test_rows_sum[B = 1, 256] / [B = 257, 300]
  fpm_rows_sum keyed, accumulate, V = 1    test_rows_sum_keyed, test_rows_sum_accumulate, test_rows_sum[K = 65]
  fpm_transpose, fpm_elementwise           test_transpose, test_elementwise
  wgrad S = 1 / split-K S = 2, 3           test_wgrad[160, 512] / [513], [1300]
  whole backward                           test_chain_bwd (NV = 40 on both blocks, TJ = 2, 3, two-level sums,
                                           split-K wgrad, keyed sum with Bu < B, the 600 cap)

The per-channel offset case of the instance norm (offset = 8 x spread) bounds the regime in which a
trained norm bias feeds the next norm: the second norm of a block reads o1 + ff, and o1 carries the
first norm's bias as a per-channel offset on a spread of |weight|.

What the stage tests found, and what was changed for it (BEFORE: the figures of the run on the
kernels as they were, same cases, same rule):

Instance-norm statistics.  The backward summed the raw values while the forward (instnorm_kernel)
sums them relative to the channel's first position x0.  With the raw sums the one-hot mode missed
the rule at every P >= 256: on the constant channels c >= nvalid xhat came out as rstd = 316 times
the rounding error of the fp32 mean instead of 0, and dw_part with it (10.0 to 11.2 times err32; the
constant channels on their own were compared only in the launches that got that far, up to 7.8).
The offset inputs passed either way.  instnorm_bwd_kernel now forms its statistics as the forward does; the constant channels give
dw_part = 0 exactly.

Attention row sum.  The kernel took S_i = sum_j exp(score - M_i) from the forward's statistics,
where it is a sum of exp2-approximated terms, and formed att = expf(score - M_i) / S_i: sum_j att = 1
then holds only to ~1e-6, and the cancelling sum sum_j dscore = 0 turns that into an error of dW2 and
dW1 of |pre-activation| ~ |b1| ~ 10 times as much with the init weights (dW2 30 to 65 times err32;
dwv_part 8.6 to 9.7).  With the statistics of the float64 reference the mismatch was larger still
(dwv_part 29 times err32): the fault was on the backward's side, in mixing two evaluations of the
softmax.  The kernel now sums its own terms in the row reduction it already had, and reads only M_i.

MEASURED: the largest device_err / err32 per stage over all cases of one run on an MI355X, after both
changes.  Where a figure exceeds 8 the floor was the gate (err32 ~ 1 ulp of a single value; the
fraction of the gate used was 0.14).  The gates do not use these numbers.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from fpm import _lib, afau_grad, afau_torch, ops
from fpm import config as C

import afau_bwd_ref as R
from test_afau_stages import DEV, MIX, ROW, _gate_check, _i32, _sd, _tailview, _weights

pytestmark = pytest.mark.gpu

MEASURED = {
    "head.dgr": 1.26, "head.dgc": 1.09, "head.dW0": 3.19, "head.db0": 6.35, "head.dw2": 1.51, "head.db2": 8.51,
    "instnorm.dense.dx": 1.71, "instnorm.dense.dw": 2.89, "instnorm.dense.db": 1.53,
    "instnorm.seed.dx": 2.35, "instnorm.seed.dw": 2.31,                 # db_part == gseed exactly
    "instnorm.onehot.dx": 3.72, "instnorm.onehot.dw": 1.95, "instnorm.onehot.db": 2.75,
    "instnorm.onehot.const.dw": 0.0,                                    # exactly 0 on the device
    "instnorm.tie.dx": 1.93, "instnorm.tie.dw": 1.54, "instnorm.acc.dx": 1.25, "instnorm.nodx.db": 1.9,
    "attn.init.dwv": 2.03, "attn.init.dW2": 0.72, "attn.init.dW1": 2.51, "attn.init.db1": 1.91,
    "attn.edge.dwv": 1.0, "attn.edge.dW2": 2.26, "attn.edge.dW1": 1.64, "attn.edge.db1": 1.25,
    "attn.init.ref.dwv": 2.03, "attn.edge.ref.dwv": 1.0,                # float64 statistics
    "wgrad": 2.03,
    # whole backward: the largest fraction of a parameter's gate (the combine bias's), max |ks - ks64|
    "chain.frac": 0.15, "chain.combine_bias.frac": 0.15, "chain.ks": 1.4e-7,
}
BEFORE = {
    "instnorm.onehot.dw": 11.2, "instnorm.onehot.const.dw": 7.8, "instnorm.offset.dense.dx": 2.6,
    "instnorm.offset.seed.dw": 2.8,
    "attn.init.dW2": 65.1, "attn.init.dwv": 9.64, "attn.edge.dwv": 9.64, "attn.edge.dW1": 7.03,
    "attn.init.ref.dwv": 29.3, "attn.edge.ref.dwv": 6.55,
}

E = C.AFAU_EMB
NAN = float("nan")


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _rule(tag, dev, ref, ref32):
    """The tolerance rule above for one output tensor."""
    ref = ref.double()
    dev = dev.detach().cpu()
    assert dev.shape == ref.shape, (tag, dev.shape, ref.shape)
    floor = 2.0 ** -20 * float(ref.abs().max())
    err32 = float((ref32.double() - ref).abs().max())
    if floor == 0.0 and err32 == 0.0:
        # both references are exactly 0: so is the exact result, and the device has to say so
        print("MEASURE %s exact-zero" % tag)
        assert torch.isfinite(dev).all() and float(dev.abs().max()) == 0.0, tag
        return
    _gate_check(tag, dev, ref, ref32, floor)


# ------------------------------------------------------------------------------------------ heads
def _head_case(B, kind):
    """(head parameters, gr, gc, dks).  "moved": two first-layer biases of each head shifted by +-5
    (units of both signs for certain); "dead": the column head's first-layer biases shifted down until
    every hidden unit is inactive."""
    sd = _sd()
    hp = {k: sd[k].clone() for k in R.HEAD_KEYS}
    g = torch.Generator().manual_seed(70 + B)
    gr = torch.rand(B, E, generator=g) * 6 - 3
    gc = torch.rand(B, E, generator=g) * 6 - 3
    for head in ("final_row", "final_col"):
        hp[head + ".0.bias"][0] += 5.0
        hp[head + ".0.bias"][1] -= 5.0
    if kind == "dead":
        hid = R.head_hidden(gr, gc, hp)
        hp["final_col.0.bias"] -= float(hid[:, 1].max()) + 5.0
    dks = torch.randn(B, generator=g)
    return hp, gr, gc, dks


@pytest.mark.parametrize("kind", ["moved", "dead"])
@pytest.mark.parametrize("B", [1, 5])
def test_head_bwd(B, kind):
    """fpm_afau_head_bwd: dgr, dgc and every parameter's per-pair partial, for d(ks) of both signs."""
    hp, gr, gc, dks0 = _head_case(B, kind)
    hid = R.head_hidden(gr, gc, hp)
    assert float(hid.abs().min()) >= 1e-3 * float(hid.abs().max())          # the ReLU margin
    assert (hid[:, 0] > 0).any() and (hid[:, 0] < 0).any()
    if kind == "dead":
        assert (hid[:, 1] < 0).all()
    else:
        assert (hid[:, 1] > 0).any() and (hid[:, 1] < 0).any()
    PS = 8 * E + 17
    d = {k: _dev(v.reshape(-1)) for k, v in hp.items()}
    for sgn in (1.0, -1.0):
        dks = dks0 * sgn
        if B > 1:
            assert (dks > 0).any() and (dks < 0).any()
        ref = R.head_bwd(gr, gc, hp, dks, torch.float64)
        ref32 = R.head_bwd(gr, gc, hp, dks, torch.float32)
        dgr, dgc, part = _nan(B, E), _nan(B, E), _nan(B, 2 * PS)
        gr_d, gc_d, dks_d = _dev(gr), _dev(gc), _dev(dks)
        _lib.call("fpm_afau_head_bwd", ops._p(gr_d), ops._p(gc_d), B, E, *[ops._p(d[k]) for k in R.HEAD_KEYS],
                  ops._p(dks_d), ops._p(dgr), ops._p(dgc), ops._p(part), ops._stream(dgr))
        torch.cuda.synchronize()
        part = part.cpu()
        _rule("head.dgr", dgr, ref[0], ref32[0])
        _rule("head.dgc", dgc, ref[1], ref32[1])
        for q, head in enumerate(("row", "col")):
            o = q * PS
            for name, a, e in (("dW0", 0, 8 * E), ("db0", 8 * E, 8 * E + 8), ("dw2", 8 * E + 8, 8 * E + 16),
                               ("db2", 8 * E + 16, 8 * E + 17)):
                _rule("head.%s.%s" % (head, name), part[:, o + a:o + e], ref[2][:, o + a:o + e], ref32[2][:, o + a:o + e])
        # an inactive unit passes nothing on: its dW0 row, db0 and dw2 are exactly 0
        off = (hid <= 0)                                                    # (B, 2, 8)
        for q in range(2):
            blk = part[:, q * PS:(q + 1) * PS]
            assert (blk[:, :8 * E].reshape(B, 8, E)[off[:, q]] == 0).all()
            assert (blk[:, 8 * E:8 * E + 8][off[:, q]] == 0).all() and (blk[:, 8 * E + 8:8 * E + 16][off[:, q]] == 0).all()
        if kind == "dead":
            assert (dgc.cpu() == 0).all() and (part[:, PS:2 * PS - 1] == 0).all()


# ------------------------------------------------------------------------------------------ instance norm
NORM_SHAPES = [(3, 1, 600), (2, 16, 600), (3, 37, 600), (2, 256, 600), (2, 257, 600), (1, 600, 600), (1, 640, 64),
               (2, 40, 70)]


def _inb(B, P, Cn, w, b, in1=None, in2=None, nvalid=None, bias=None, dy=None, gseed=None, dx="new", accumulate=0):
    """fpm_instnorm_bwd on CPU operands -> (dx, dw_part, db_part) on the device, outputs pre-filled
    with NaN (``dx``: "new", None for a null pointer, or a pre-filled device tensor)."""
    t = [_dev(x) for x in (in1, in2, bias, w, b, dy, gseed)]
    nv = None if nvalid is None else _i32(nvalid)
    dxd = _nan(B * P, Cn) if isinstance(dx, str) else dx
    dwp, dbp = _nan(B, Cn), _nan(B, Cn)
    _lib.call("fpm_instnorm_bwd", ops._p(t[0]), ops._p(t[1]), B, P, Cn, ops._p(nv), ops._p(t[2]), ops._p(t[3]),
              ops._p(t[4]), float(C.IN_EPS), ops._p(t[5]), ops._p(t[6]), ops._p(dxd), int(accumulate), ops._p(dwp),
              ops._p(dbp), ops._stream(dwp))
    torch.cuda.synchronize()
    return dxd, dwp, dbp


def _bumped(x1, x2, w, b, g, tie=None):
    """x2 changed so that x1 + x2 has, per (pair, channel), its maximum at a chosen position, 0.5 above
    the rest (w > 0: also the maximum of y); ``tie``: (p, q) -> every channel's maximum sits at both
    positions, exactly equal.  Asserts the top-2 gap of y in float64 (>= 1e-3 of the channel's spread;
    for a tie: the third value that far below)."""
    B, P, Cn = x1.shape
    x2 = x2.clone()
    if P == 1:
        return x2, torch.zeros(B, Cn, dtype=torch.long)
    top = (x1 + x2).max(dim=1).values + 0.5
    if tie is None:
        pm = torch.randint(0, P, (B, Cn), generator=g)
        val = (top - x1.gather(1, pm[:, None, :])[:, 0]).float()
        x2.scatter_(1, pm[:, None, :], val[:, None, :])
    else:
        # equal fp32 sums: x1 = 0 at both positions, x2 = the same value
        for p in tie:
            x1[:, p, :] = 0.0
            x2[:, p, :] = top
        pm = torch.full((B, Cn), min(tie), dtype=torch.long)
    y = R.instnorm_fwd(x1.double() + x2.double(), w, b)
    srt = y.sort(dim=1, descending=True).values
    k = 1 if tie is None else 2
    if tie is not None:
        assert torch.equal(srt[:, 0], srt[:, 1])
    assert ((srt[:, 0] - srt[:, k]) >= 1e-3 * (srt[:, 0] - srt[:, -1])).all()
    assert torch.equal(R.pool_argmax(y), pm)
    return x2, pm


def _norm_params(P, Cn, salt=0):
    g = torch.Generator().manual_seed(2000 * P + Cn + salt)
    return g, torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g) * 0.1


def _check_norm(tag, got, x64, x32, w, b, B, P, Cn, dy=None, gseed=None, want_dx=True):
    ref = R.instnorm_bwd(x64, w, b, dy=dy, gseed=gseed, dtype=torch.float64)
    ref32 = R.instnorm_bwd(x32, w, b, dy=dy, gseed=gseed, dtype=torch.float32)
    if want_dx:
        _rule(tag + ".dx", got[0].view(B, P, Cn), ref[0], ref32[0])
    _rule(tag + ".dw", got[1], ref[1], ref32[1])
    _rule(tag + ".db", got[2], ref[2], ref32[2])
    if gseed is not None:
        assert torch.equal(got[2].cpu(), gseed)             # the seed lands on one position, whole
    return ref, ref32


@functools.lru_cache(maxsize=None)
def _norm_cases(B, P, Cn):
    """(w, b, cases) of one shape; a case: tag, the kernel's operands ``call``, the norm's input in
    float64 / float32 (x64 / x32), and for the one-hot mode ``nvalid``.  Unit-normal inputs and inputs
    with a per-channel offset of 8 times their spread, each as in1 with a dense dy and as in1 + in2 with
    the max pool's seed; the one-hot input with nvalid = 0, P / 2 and P in every pair's turn."""
    g, w, b = _norm_params(P, Cn)
    cases = []
    for kind in ("normal", "offset"):
        off = 8.0 * torch.where(torch.arange(Cn) % 2 == 0, 1.0, -1.0) if kind == "offset" else torch.zeros(Cn)
        x1 = torch.randn(B, P, Cn, generator=g) + off
        dy = torch.randn(B, P, Cn, generator=g)
        cases.append(dict(tag="instnorm.%s.dense" % kind, call=dict(in1=x1, dy=dy), x64=x1.double(), x32=x1))
        x2, _ = _bumped(x1, torch.randn(B, P, Cn, generator=g), w, b, g)
        gs = torch.randn(B, Cn, generator=g)
        cases.append(dict(tag="instnorm.%s.seed" % kind, call=dict(in1=x1, in2=x2, gseed=gs),
                          x64=x1.double() + x2.double(), x32=x1 + x2))
    bias = torch.randn(Cn, generator=g) * 0.1
    for turn in range(3):
        nvalid = [(0, P // 2, P)[(turn + i) % 3] for i in range(B)]
        dy = torch.randn(B, P, Cn, generator=g)
        cases.append(dict(tag="instnorm.onehot", call=dict(nvalid=nvalid, bias=bias, dy=dy), nvalid=nvalid,
                          x64=R.onehot_input(B, P, Cn, nvalid, bias, torch.float64),
                          x32=R.onehot_input(B, P, Cn, nvalid, bias, torch.float32)))
    return w, b, cases


@pytest.mark.parametrize("B,P,Cn", NORM_SHAPES, ids=["%dx%dx%d" % s for s in NORM_SHAPES])
def test_instnorm_bwd(B, P, Cn):
    """fpm_instnorm_bwd in the modes the backward uses: in1 with a dense dy (first norm of the row
    block), in1 + in2 with the max pool's seed (second norm), the synthesised one-hot input with a dense
    dy (first norm of the column block)."""
    w, b, cases = _norm_cases(B, P, Cn)
    for cs in cases:
        got = _inb(B, P, Cn, w, b, **cs["call"])
        ref, ref32 = _check_norm(cs["tag"], got, cs["x64"], cs["x32"], w, b, B, P, Cn, dy=cs["call"].get("dy"),
                                 gseed=cs["call"].get("gseed"))
        if "nvalid" not in cs:
            continue
        # the constant channels c >= nvalid on their own: xhat = 0 there, so the exact dw_part is 0
        const = torch.arange(Cn)[None, :] >= torch.tensor(cs["nvalid"])[:, None]
        if P == 1:
            const = torch.ones(B, Cn, dtype=torch.bool)
        if not const.any():
            continue
        assert float(ref[1][const].abs().max()) < 1e-9
        _rule("instnorm.onehot.const.dw", got[1].cpu()[const], torch.zeros(int(const.sum())), ref32[1][const])


TIE_CASES = ((2, 37, 600, (20, 3)), (1, 300, 70, (260, 5)))


@functools.lru_cache(maxsize=None)
def _tie_case(B, P, Cn, tie):
    """Every channel's maximum of in1 + in2 at both positions of ``tie``, exactly equal."""
    assert tie[0] % 16 != tie[1] % 16
    g, w, b = _norm_params(P, Cn, 1)
    x1 = torch.randn(B, P, Cn, generator=g)
    x2, _ = _bumped(x1, torch.randn(B, P, Cn, generator=g), w, b, g, tie=tie)
    gs = torch.randn(B, Cn, generator=g) + 3.0
    return w, b, x1, x2, gs


def test_instnorm_bwd_tie():
    """An exact two-way tie of the max at positions of different position groups (and, for P = 300, of
    different register slots): the seed goes to the smaller position."""
    for B, P, Cn, tie in TIE_CASES:
        w, b, x1, x2, gs = _tie_case(B, P, Cn, tie)
        got = _inb(B, P, Cn, w, b, in1=x1, in2=x2, gseed=gs)
        _check_norm("instnorm.tie", got, x1.double() + x2.double(), x1 + x2, w, b, B, P, Cn, gseed=gs)


def test_instnorm_bwd_accumulate():
    """accumulate = 1: dx holds the pre-fill plus the gradient (the same gradient, added once)."""
    B, P, Cn = 3, 37, 600
    g, w, b = _norm_params(P, Cn, 2)
    x1 = torch.randn(B, P, Cn, generator=g)
    dy = torch.randn(B, P, Cn, generator=g)
    pre = torch.randn(B * P, Cn, generator=g)
    plain = _inb(B, P, Cn, w, b, in1=x1, dy=dy)
    acc = _inb(B, P, Cn, w, b, in1=x1, dy=dy, dx=pre.to(DEV), accumulate=1)
    assert torch.equal(acc[0].cpu(), pre + plain[0].cpu())
    assert torch.equal(acc[1], plain[1]) and torch.equal(acc[2], plain[2])
    ref = R.instnorm_bwd(x1.double(), w, b, dy=dy, dtype=torch.float64)
    ref32 = R.instnorm_bwd(x1, w, b, dy=dy, dtype=torch.float32)
    _rule("instnorm.acc.dx", acc[0].view(B, P, Cn), pre.view(B, P, Cn).double() + ref[0],
          pre.view(B, P, Cn) + ref32[0])


def test_instnorm_bwd_no_dx():
    """dx = null (want_dx = False, the column block's first norm): only the partials are written."""
    B, P = 2, 40
    g, w, b = _norm_params(P, E, 3)
    bias = torch.randn(E, generator=g) * 0.1
    dy = torch.randn(B, P, E, generator=g)
    nvalid = [P, 17]
    got = _inb(B, P, E, w, b, nvalid=nvalid, bias=bias, dy=dy, dx=None)
    assert got[0] is None
    _check_norm("instnorm.nodx", got, R.onehot_input(B, P, E, nvalid, bias, torch.float64),
                R.onehot_input(B, P, E, nvalid, bias, torch.float32), w, b, B, P, E, dy=dy, want_dx=False)
    # the same through afau_grad's wrapper: partials summed over the pairs
    dx, gw, gb = afau_grad._instnorm_bwd(None, None, B, P, nvalid=_i32(nvalid), onehot_bias=_dev(bias), w=_dev(w),
                                         b=_dev(b), dy=_dev(dy.view(B * P, E)), want_dx=False)
    torch.cuda.synchronize()
    assert dx is None
    assert torch.equal(gw.cpu(), (got[1][0] + got[1][1]).cpu()) and torch.equal(gb.cpu(), (got[2][0] + got[2][1]).cpu())


def test_instnorm_bwd_rejections():
    """641 positions, both seeds, no seed: refused on the host, nothing launched (outputs untouched)."""
    w = torch.ones(64)
    for P, both, neither in ((641, False, False), (40, True, False), (40, False, True)):
        x = torch.zeros(1, P, 64)
        dy = None if neither else x
        gs = torch.zeros(1, 64) if both else None
        dxd = _nan(P, 64)
        with pytest.raises(_lib.FpmError):
            _inb(1, P, 64, w, w, in1=x, dy=dy, gseed=gs, dx=dxd)
        torch.cuda.synchronize()
        assert torch.isnan(dxd).all()


# ------------------------------------------------------------------------------------------ attention
ATTN_SHAPES = [
    (3, 37, 45, [45, 20, 1]),       # a ragged batch
    (2, 8, 256, [256, 255]),        # the TJ = 1 edge
    (2, 8, 257, [257, 130]),        # the first TJ = 2
    (1, 8, 512, [512]),             # the TJ = 2 edge
    (1, 8, 513, [513]),             # the first TJ = 3
    (1, 6, 600, [600]),             # the cap
]
# cost: "soft" a doubly-stochastic-like softmax; "view" a row-strided view of a wider buffer (c_ld);
# "pad" rows of zeros where a pair has fewer rows than the box; "ref": "soft" with the softmax
# statistics taken from the float64 reference rounded to fp32 instead of the forward kernel
ATTN_CASES = [(0, "soft"), (0, "pad"), (0, "ref"), (1, "view"), (2, "soft"), (3, "view"), (4, "soft"), (5, "soft")]
ATTN_KEYS = (ROW + ".Wv.weight", MIX + "mix1_weight", MIX + "mix1_bias", MIX + "mix2_weight", MIX + "mix2_bias")


def _near_kinks(cost, w1, b1):
    """(entries whose pre-activation is within 2^-20 (|c w1| + |b1|) of the kink without being exactly
    0, entries exactly 0 whose fp32 evaluation is not certain to be 0 too)."""
    pre = R.attn_pre(cost, w1, b1)
    c, ww, bb = cost.double()[:, None, :, :, None], w1.double()[None, :, 1, None, None, :], \
        b1.double()[None, :, None, None, :]
    near = (pre != 0) & (pre.abs() < 2.0 ** -20 * ((c * ww).abs() + bb.abs()))
    prod32 = cost[:, None, :, :, None] * w1[None, :, 1, None, None, :]
    unsure = (pre == 0) & ((prod32.double() != c * ww) | ((prod32 + b1[None, :, None, None, :]) != 0))
    return int(near.sum()), int(unsure.sum()), int((pre == 0).sum())


@functools.lru_cache(maxsize=None)
def _attn_case(si, variant, wkind):
    B, n1max, n2max, n2s = ATTN_SHAPES[si]
    wsd = _weights(wkind)
    Wv, w1, b1, w2, b2 = (wsd[k] for k in ATTN_KEYS)
    n1s = [n1max, max(1, n1max - 7), 5][:B] if variant == "pad" else [n1max] * B
    base = 5000 + 100 * si + (7 if wkind == "edge" else 0)
    for seed in range(base, base + 50):             # the first seed without a pre-activation near its kink
        g = torch.Generator().manual_seed(seed)
        cost = torch.zeros(B, n1max, n2max)
        for bi in range(B):
            cost[bi, :n1s[bi], :n2s[bi]] = torch.softmax(torch.randn(n1s[bi], n2s[bi], generator=g) * 3, dim=1)
        if wkind == "edge":
            # costs exactly on the constructed breakpoints: 0, 0.5, 1 (head 3) and the bucket edges 4 m / 64 (head 1)
            cost[0, 0, 0] = 1.0
            k = min(n2s[0], 16)
            cost[0, 1, :k] = (4 * torch.arange(16, dtype=torch.float32) / 64)[:k]
            cost[0, 2, 0], cost[0, 2, 1] = 0.5, 0.0
        near, unsure, zeros = _near_kinks(cost, w1, b1)
        if near == 0:
            break
    assert near == 0 and unsure == 0
    if wkind == "edge":
        assert zeros > 0 and float(cost.min()) >= 0.0 and float(cost.max()) <= 1.0
    datt = torch.randn(B * n1max, 256, generator=g)
    ref = R.attn_bwd(cost, n2s, Wv, w1, b1, w2, b2, datt, torch.float64)
    ref32 = R.attn_bwd(cost, n2s, Wv, w1, b1, w2, b2, datt, torch.float32)
    stats64 = R.attn_fwd(cost, n2s, Wv, w1, b1, w2, b2)[1].float() if variant == "ref" else None
    return cost, datt, ref, ref32, stats64


@pytest.mark.parametrize("wkind", ["init", "edge"])
@pytest.mark.parametrize("si,variant", ATTN_CASES, ids=["%d-%s" % (ATTN_SHAPES[i][2], v) for i, v in ATTN_CASES])
def test_attn_bwd(si, variant, wkind):
    """fpm_afau_attn_bwd with the forward kernel's softmax statistics (the production pairing) against
    the float64 attention backward: dwv_part, and dW2 / dW1 / db1 per parameter tensor."""
    B, n1max, n2max, n2s = ATTN_SHAPES[si]
    cost, datt, ref, ref32, stats64 = _attn_case(si, variant, wkind)
    wsd = _weights(wkind)
    w = [wsd[k].to(DEV).contiguous() for k in ATTN_KEYS]
    if variant == "view":
        buf = torch.full((B, n1max, n2max + 4), 0.5, device=DEV)
        cost_d = buf[:, :, :n2max]
        cost_d.copy_(cost)
        assert not cost_d.is_contiguous()
    else:
        cost_d = cost.to(DEV)
    n2_d = _i32(n2s)
    rows = B * n1max
    att, st = _nan(rows, 256), _nan(rows, 16, 2)
    ops.crossset_attn(cost_d, n2_d, *w, att, stats=st)
    if stats64 is not None:
        st = stats64.to(DEV).contiguous()
    datt_d = datt.to(DEV)
    dwvp, mixp = _nan(B, 256, n2max), _nan(B, 16, 49)
    _lib.call("fpm_afau_attn_bwd", ops._p(cost_d), cost_d.stride(0), cost_d.stride(1), B, n1max, n2max, ops._p(n2_d),
              ops._p(w[0]), w[0].shape[1], ops._p(w[1]), ops._p(w[2]), ops._p(w[3]), ops._p(w[4]), ops._p(att),
              ops._p(datt_d), ops._p(st), ops._p(dwvp), ops._p(mixp), ops._stream(datt_d))
    torch.cuda.synchronize()
    dwvp, mixp = dwvp.cpu(), mixp.cpu()
    tag = "attn.%s.%s" % (wkind, "ref" if variant == "ref" else "fwd")
    _rule(tag + ".dwv", dwvp, ref[0], ref32[0])
    for name, a in (("dW2", 0), ("dW1", 16), ("db1", 32)):
        _rule("%s.%s" % (tag, name), mixp[:, :, a:a + 16], ref[1][:, :, a:a + 16], ref32[1][:, :, a:a + 16])
    for bi in range(B):
        assert (dwvp[bi, :, n2s[bi]:] == 0).all()           # v = 0 beyond n2: exactly no gradient
    assert (mixp[:, :, 48] == 0).all()                      # mix2_bias shifts every score of a head
    assert float(ref[1][:, :, 48].abs().max()) <= 1e-12 * float(ref[1].abs().max())
    if wkind == "edge":
        # head 4: every breakpoint outside [0, 1], so each unit is active on all costs or on none:
        # the sum over the fewer entries is empty and db1 is exactly 0
        assert (mixp[:, 4, 32:48] == 0).all()


def test_attn_bwd_rejections():
    wsd = _weights("init")
    w = [wsd[k].to(DEV).contiguous() for k in ATTN_KEYS]
    for n2max, emb in ((769, 800), (45, 40)):
        cost = torch.zeros(1, 2, n2max, device=DEV)
        dwvp, mixp = _nan(1, 256, n2max), _nan(1, 16, 49)
        z = torch.zeros(2, 256, device=DEV)
        st = torch.ones(2, 16, 2, device=DEV)
        n2_d = _i32([n2max])
        with pytest.raises(_lib.FpmError):
            _lib.call("fpm_afau_attn_bwd", ops._p(cost), cost.stride(0), cost.stride(1), 1, 2, n2max, ops._p(n2_d),
                      ops._p(w[0]), emb, ops._p(w[1]), ops._p(w[2]), ops._p(w[3]), ops._p(w[4]), ops._p(z), ops._p(z),
                      ops._p(st), ops._p(dwvp), ops._p(mixp), ops._stream(cost))
        torch.cuda.synchronize()
        assert torch.isnan(dwvp).all() and torch.isnan(mixp).all()


# ------------------------------------------------------------------------------------------ the glue
def _dyadic(g, *shape):
    """Multiples of 1 / 8 in [-8, 8]: every partial sum of fewer than 2^16 of them is exact in fp32."""
    return torch.randint(-64, 65, shape, generator=g).float() / 8


@pytest.mark.parametrize("K", [(64,), (5, 13)], ids=["K64", "K65"])
@pytest.mark.parametrize("B", [1, 256, 257, 300])
def test_rows_sum(B, K):
    """afau_grad.rows_sum without keys (B > 256: two levels) on dyadic values, where every order of
    summation is exact: equal to the float64 sum.  K = 65: the one-value-per-thread form."""
    g = torch.Generator().manual_seed(B + len(K))
    x = _dyadic(g, B, *K)
    out = afau_grad.rows_sum(x.to(DEV))
    torch.cuda.synchronize()
    assert out.shape == tuple(K)
    assert torch.equal(out.cpu().double(), R.rows_sum(x))


@pytest.mark.parametrize("K", [64, 65])
def test_rows_sum_keyed(K):
    """With keys: out[u] sums the rows with key u; a key no row carries gives a row of zeros."""
    g = torch.Generator().manual_seed(K)
    x = _dyadic(g, 9, K)
    key = [0, 3, 0, 3, 3, 1, 0, 1, 3]                      # key 2 is empty
    out = afau_grad.rows_sum(x.to(DEV), key=_i32(key), nkeys=4)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().double(), R.rows_sum(x, key=key, nkeys=4))
    assert (out[2] == 0).all()


@pytest.mark.parametrize("K", [64, 65])
def test_rows_sum_accumulate(K):
    """accumulate = 1 (fpm_rows_sum called directly): the sums are added to what out holds."""
    g = torch.Generator().manual_seed(10 + K)
    x, pre = _dyadic(g, 20, K), _dyadic(g, 3, K)
    key = [k % 3 for k in range(20)]
    xd, out, kd = x.to(DEV), pre.to(DEV), _i32(key)
    _lib.call("fpm_rows_sum", ops._p(xd), 20, K, ops._p(kd), 3, ops._p(out), 1, ops._stream(xd))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().double(), pre.double() + R.rows_sum(x, key=key, nkeys=3))


@pytest.mark.parametrize("Rr,Cc,ldo", [(33, 31, 36), (300, 600, 300), (5, 1, 8)])
def test_transpose(Rr, Cc, ldo):
    """afau_grad.transpose: exact values, columns [R, ldo) exactly 0, for a contiguous input and for a
    column slice of a wider buffer (ldi > C)."""
    g = torch.Generator().manual_seed(Rr)
    x = torch.randn(Rr, Cc, generator=g)
    wide = torch.full((Rr, Cc + 3), NAN, device=DEV)
    view = wide[:, :Cc]
    view.copy_(x)
    assert view.stride(0) == Cc + 3
    for xd in (x.to(DEV), view):
        out = afau_grad.transpose(xd, ldo)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), R.transpose_pad(x, ldo))


def test_elementwise():
    """afau_grad._ew: mode 0 the ReLU mask, mode 1 the add, exact; n = 1000 is no multiple of the block
    size.  Another mode is refused and leaves x alone."""
    g = torch.Generator().manual_seed(8)
    x, ref = torch.randn(1000, generator=g), torch.randn(1000, generator=g)
    ref[::7] = 0.0                                          # post-activations that are exactly 0
    assert torch.equal(afau_grad._ew(x.to(DEV), ref.to(DEV), 0).cpu(), R.relu_mask(x, ref))
    assert torch.equal(afau_grad._ew(x.to(DEV), ref.to(DEV), 1).cpu(), R.add(x, ref))
    xd = x.to(DEV)
    with pytest.raises(_lib.FpmError):
        afau_grad._ew(xd, ref.to(DEV), 2)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x)


@pytest.mark.parametrize("Rr", [160, 512, 513, 1300])
def test_wgrad(Rr):
    """afau_grad.wgrad (transposes, batched fp32 product over S = ceil(R / 512) slices of the rows,
    in-order sum of the slices) against dY^T X in float64."""
    N1, N2 = 600, 256
    g = torch.Generator().manual_seed(Rr)
    dY, X = torch.randn(Rr, N1, generator=g), torch.randn(Rr, N2, generator=g)
    X = torch.relu(X)                                        # as the FFN's hidden rows: half of them 0
    out = afau_grad.wgrad(dY.to(DEV), X.to(DEV))
    torch.cuda.synchronize()
    _rule("wgrad", out, R.wgrad(dY, X), R.wgrad(dY, X, torch.float32))


# ------------------------------------------------------------------------------------------ whole backward
CHAIN_CASES = [
    ((300,), (270,)),                                        # NV = 40 on both blocks, TJ = 2, two-level rows_sum
    ((128,) * 5, (128, 101, 128, 101, 128)),                 # 640 rows: split-K wgrad S = 2; Bu < B: the keyed sum
    ((40,), (520,)),                                         # TJ = 3, column block with P = 520
    ((600,), (600,)),                                        # the cap
]
ZERO_WRITTEN = ("Wq.weight", "Wk.weight", "col_encoding_block.Wv.weight", "col_encoding_block.multi_head_combine.weight",
                "col_encoding_block.multi_head_combine.bias", "col_encoding_block.mixed_score_MHA.mix1_weight",
                "col_encoding_block.mixed_score_MHA.mix1_bias", "col_encoding_block.mixed_score_MHA.mix2_weight",
                "mixed_score_MHA.mix2_bias")
ROW_COMBINE_BIAS = "encoder_k.layers.0.row_encoding_block.multi_head_combine.bias"


class _GrabCombine(torch.overrides.TorchFunctionMode):
    """Keeps the output of the product with ``weight`` (the row block's combine) of a replay, its
    gradient retained: d(mh), whose sum over the rows is the combine bias's gradient."""

    def __init__(self, weight):
        super().__init__()
        self.weight, self.mh = weight, []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if func is F.linear and args[1] is self.weight:
            out.retain_grad()
            self.mh.append(out)
        return out


def _group(k):
    return k.split(".")[0] + ("." + k.split(".")[3] if k.startswith("encoder_k") else "")


def _replay(ss, n1s, n2s, prm, dks, dtype):
    """Autograd through fpm.afau_torch.afau_ks on the device in ``dtype`` -> (ks, gradients, d(mh) of the row block)."""
    leaves = {k: v.to(dtype).clone().requires_grad_(True) for k, v in prm.items()}
    with _GrabCombine(leaves[ROW_COMBINE_BIAS[:-4] + "weight"]) as grab:
        ks = afau_torch.afau_ks(ss.to(dtype), torch.tensor(n1s, device=DEV), torch.tensor(n2s, device=DEV),
                                lambda k: leaves[k])
        (ks * dks.to(dtype)).sum().backward()
    assert len(grab.mh) == 1
    return ks.detach(), {k: v.grad for k, v in leaves.items()}, grab.mh[0].grad


@pytest.mark.parametrize("x3", [False, True], ids=["f32", "x3"])
@pytest.mark.parametrize("n1s,n2s", CHAIN_CASES, ids=["300x270", "5x128", "40x520", "600x600"])
def test_chain_bwd(n1s, n2s, x3):
    """afau_grad.forward + backward against autograd through the replay in float64 on the device (the
    fp32 replay is the ref32): every parameter tensor within max(2e-3 x its group's scale -- the
    project's chain bound --, 8 |replay32 - replay64|); zeros where the code writes zeros; the row
    block's combine bias (a cancelling sum over all rows, exact value 0) within
    max(8 |replay32's value|, 2^-20 sum|d(mh)|)."""
    sd = _sd()
    g = torch.Generator().manual_seed(sum(n1s) + sum(n2s))
    B, n1max, n2max = len(n1s), max(n1s), max(n2s)
    ss = torch.zeros(B, n1max, n2max)
    for b in range(B):
        ss[b, :n1s[b], :n2s[b]] = torch.softmax(torch.randn(n1s[b], n2s[b], generator=g) * 3, dim=1)
    names = [k for k in sd if k.startswith(afau_torch.AFAU_PARAM_PREFIXES) and sd[k].is_floating_point()]
    prm = {k: sd[k].to(DEV).float() for k in names}
    ssd = ss.to(DEV)
    dks = torch.randn(B, generator=g).to(DEV)
    ks, sv = afau_grad.forward(lambda k: prm[k], ssd, _tailview(list(n1s), list(n2s)), x3=x3)
    grads = dict(zip(names, afau_grad.backward(lambda k: prm[k], sv, dks, names)))
    torch.cuda.synchronize()
    ks64, g64, dmh = _replay(ssd, n1s, n2s, prm, dks, torch.float64)
    _, g32, _ = _replay(ssd, n1s, n2s, prm, dks, torch.float32)
    kerr = float((ks.double() - ks64).abs().max())
    print("MEASURE chain.ks err=%.3g" % kerr)
    assert kerr < 1e-4                                       # the forward chain's bound (test_afau_stages)
    scale = {}
    for k in names:
        if g64[k] is not None:
            scale[_group(k)] = max(scale.get(_group(k), 0.0), float(g64[k].abs().max()))
    bad = []
    for k in names:
        got = grads[k]
        assert torch.isfinite(got).all(), k
        if k.endswith(ZERO_WRITTEN):
            assert float(got.abs().max()) == 0.0, k
            continue
        ref = g64[k]
        err32 = float((g32[k].double() - ref).abs().max())
        if k == ROW_COMBINE_BIAS:
            gate = torch.clamp(2.0 ** -20 * dmh.abs().sum(dim=(0, 1)), min=8.0 * float(g32[k].abs().max()))
            err = (got.double() - ref).abs()
            frac = float((err / gate).max())
            print("MEASURE chain.combine_bias err=%.3g replay32=%.3g gate=%.3g frac=%.3g"
                  % (float(err.max()), float(g32[k].abs().max()), float(gate.max()), frac))
        else:
            if k.endswith("mixed_score_MHA.mix1_weight"):
                assert float(got[:, 0].abs().max()) == 0.0, k       # the zero dot product's row
            gate = max(2e-3 * scale[_group(k)], 8.0 * err32)
            err = float((got.double() - ref).abs().max())
            frac = err / gate
            print("MEASURE chain.%s err=%.3g err32=%.3g gate=%.3g frac=%.3g" % (k.split("layers.0.")[-1], err, err32,
                                                                              gate, frac))
        if not frac <= 1.0:
            bad.append((k, frac))
    assert not bad, bad


def test_chain_cap():
    """601 keypoints are past UNIV_SIZE: afau_grad.forward refuses before any kernel runs."""
    sd = _sd()
    with pytest.raises(AssertionError):
        afau_grad.forward(lambda k: sd[k].to(DEV), torch.zeros(1, 601, 8, device=DEV), _tailview([601], [8]))

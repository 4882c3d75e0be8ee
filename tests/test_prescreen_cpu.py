"""Prescreen of a 1:N identification, host side (no GPU): the host statements of ``ops.rows_pool`` (a template's
pooled descriptor) and ``ops.rank_keep`` (the k best of a row, any k, in entry order) against plain numpy
restatements of their definitions, and the refusals of bad arguments.

The helpers here (the ragged pool case, the quantised score rows, the numpy statements) also serve
``test_prescreen_gpu.py``."""
import numpy as np
import pytest
import torch

from fpm import _lib, ops

POOL_NS = (1, 2, 17, 128, 600, 5)          # the last entry is all zeros
# (P, G, k): one column, a tie class over the threshold, k = G - 0, both sides of rank_select's 1024, slices of one
# and several workgroups, a large k
KEEP_SHAPES = [(1, 1, 1), (2, 300, 7), (3, 1023, 1023), (2, 1025, 1024), (2, 5000, 1500), (1, 100000, 40000)]


def pool_case(seed=11):
    """A ragged row store with entries of POOL_NS rows -> (y (R, 768) fp32, row_off (G + 1,) int64)."""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randn(n, 768, generator=g) * (0.5 + e) for e, n in enumerate(POOL_NS)]
    rows[-1] = torch.zeros(POOL_NS[-1], 768)
    rows[1][:, 7] = -0.0
    off = torch.tensor(np.concatenate([[0], np.cumsum(POOL_NS)]), dtype=torch.int64)
    return torch.cat(rows).contiguous(), off


def bf16_rne_numpy(x):
    """fp32 array -> the bits of the nearest bf16 (ties to even) as uint16; finite values."""
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def pool_numpy(y, off):
    """The definition of the descriptor, entry by entry, row by row -> ((E, 768) uint16 bf16 bits, (E, 768) fp64
    descriptors before the two roundings)."""
    E = len(off) - 1
    bits = np.zeros((E, 768), np.uint16)
    exact = np.zeros((E, 768), np.float64)
    for e in range(E):
        m = np.zeros(768, np.float32)
        for i in range(off[e], off[e + 1]):
            m = (m + y[i]).astype(np.float32)
        md = m.astype(np.float64)
        sq = md * md
        p = np.zeros(256, np.float64)
        for t in range(192):
            p[t] = ((sq[4 * t] + sq[4 * t + 1]) + sq[4 * t + 2]) + sq[4 * t + 3]
        o = 128
        while o:
            for t in range(o):
                p[t] = p[t] + p[t + o]
            o //= 2
        ss = p[0]
        if ss == 0 or not np.isfinite(ss):
            continue
        exact[e] = md / np.sqrt(ss)
        bits[e] = bf16_rne_numpy(exact[e].astype(np.float32))
    return bits, exact


def keep_scores(P, G, seed):
    """Scores on 16 levels (the k-th key falls inside a tie class) with a few NaN and -inf planted."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(0, 16, (P, G), generator=g).to(torch.float32) / 8 - 1
    if G > 8:
        s[:, 3] = float("nan")
        s[:, G - 2] = float("nan")
        s[0, 5] = float("-inf")
        s[-1, G // 2] = float("-inf")
        s[-1, 6] = -0.0
    return s


def key_numpy(s):
    u = s.view(np.uint32).astype(np.uint64)
    bits = np.where(u >= 0x80000000, 0xFFFFFFFF - u, u + 0x80000000)
    bits = np.where(np.isnan(s), 0, bits).astype(np.uint64)
    return (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(s.shape[1], dtype=np.uint64)[None, :])


def keep_numpy(s, k):
    """Sort by the numpy key, take k, sort the columns."""
    order = np.argsort(np.uint64(0xFFFFFFFFFFFFFFFF) - key_numpy(s), axis=1, kind="stable")[:, :k]
    return np.sort(order, axis=1).astype(np.int32)


def test_rows_pool_host_vs_numpy():
    y, off = pool_case()
    d = ops.rows_pool(y, off)
    assert d.dtype == torch.bfloat16 and tuple(d.shape) == (len(POOL_NS), 768)
    bits, exact = pool_numpy(y.numpy(), off.numpy())
    assert np.array_equal(d.view(torch.int16).numpy().view(np.uint16), bits)
    norm = np.sqrt((exact * exact).sum(1))
    assert np.all(np.abs(norm[:-1] - 1.0) < 1e-12), norm
    assert not bits[-1].any() and bits[:-1].any(1).all()
    # a sub-range and single entries: an entry's descriptor depends on its own rows alone
    sub = ops.rows_pool(y, off, 2, 5)
    assert torch.equal(sub.view(torch.int16), d[2:5].view(torch.int16))
    for e in range(len(POOL_NS)):
        one = ops.rows_pool(y, off, e, e + 1)
        assert torch.equal(one.view(torch.int16), d[e:e + 1].view(torch.int16)), e
    assert tuple(ops.rows_pool(y, off, 3, 3).shape) == (0, 768)


def test_rows_pool_non_finite_is_zero():
    y, off = pool_case()
    y = y.clone()
    y[0, 5] = float("inf")                 # entry 0
    y[1, 9] = float("nan")                 # entry 1
    y[3:20] = 3e38                         # entry 2: the fp32 sums overflow
    d = ops.rows_pool(y, off)
    assert not bool(d[:3].view(torch.int16).any()) and bool(d[3].view(torch.int16).any())


@pytest.mark.parametrize("P,G,k", KEEP_SHAPES)
def test_rank_keep_host_vs_numpy(P, G, k):
    s = keep_scores(P, G, 31 * G + k)
    keep = ops.rank_keep(s, k)
    assert keep.dtype == torch.int32 and tuple(keep.shape) == (P, k)
    assert np.array_equal(keep.numpy(), keep_numpy(s.numpy(), k))
    assert bool((keep[:, 1:] > keep[:, :-1]).all()) and int(keep.min()) >= 0 and int(keep.max()) < G
    if k <= ops.RANK_SELECT_KMAX:
        ti, _ = ops.rank_select(s, k)
        assert torch.equal(torch.sort(ti, dim=1).values, keep)
    wide = torch.zeros(P, G + 9)
    wide[:, 4:4 + G] = s
    assert torch.equal(ops.rank_keep(wide[:, 4:4 + G], k), keep)
    out = torch.full((P, k), -1, dtype=torch.int32)
    assert ops.rank_keep(s, k, keep=out) is out and torch.equal(out, keep)
    # a row stride below G (one row seen three times: stride 0) is taken through a copy
    assert torch.equal(ops.rank_keep(s[:1].expand(3, -1), k), keep[:1].expand(3, -1))


def test_desc_score_host_statement():
    g = torch.Generator().manual_seed(3)
    dq = torch.nn.functional.normalize(torch.randn(3, 768, generator=g), dim=1).to(torch.bfloat16)
    dg = torch.nn.functional.normalize(torch.randn(9, 768, generator=g), dim=1).to(torch.bfloat16)
    ref = dq.double() @ dg.double().t()
    s64 = ops.desc_score(dq, dg, dtype=torch.float64)
    s32 = ops.desc_score(dq, dg)
    assert s32.dtype == torch.float32 and tuple(s32.shape) == (3, 9)
    assert float((s64 - ref).abs().max()) < 1e-14 and float((s32.double() - ref).abs().max()) < 1e-5
    idx = torch.tensor([7, 0, 7, 2], dtype=torch.int32)
    assert torch.equal(ops.desc_score(dq, dg, idx).view(torch.int32), s32[:, idx.long()].contiguous().view(torch.int32))


def test_bad_arguments():
    s = torch.zeros(2, 50)
    for k in (0, 51, -1):
        with pytest.raises(_lib.FpmError, match="rank_keep: k"):
            ops.rank_keep(s, k)
    for bad in (s.double(), s[0], s.to(torch.bfloat16), [[0.0]]):
        with pytest.raises(_lib.FpmError, match="fp32"):
            ops.rank_keep(bad, 1)
    with pytest.raises(_lib.FpmError, match="keep"):
        ops.rank_keep(s, 3, keep=torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(_lib.FpmError, match="keep"):
        ops.rank_keep(s, 3, keep=torch.zeros(2, 4, dtype=torch.int32))
    y, off = pool_case()
    for kw, msg in ((dict(y=y.double()), "fp32"), (dict(y=y[:, :700]), "768"), (dict(row_off=off.int()), "int64"),
                    (dict(lo=4, hi=3), "outside"), (dict(hi=len(POOL_NS) + 1), "outside"), (dict(lo=-1), "outside"),
                    (dict(row_off=off.flip(0)), "rise"), (dict(row_off=off[:-1]), "rise"),
                    (dict(out=torch.zeros(len(POOL_NS), 768)), "bfloat16"),
                    (dict(out=torch.zeros(2, 768, dtype=torch.bfloat16)), "shape")):
        a = dict(y=y, row_off=off, lo=0, hi=None, out=None)
        a.update(kw)
        with pytest.raises(_lib.FpmError, match=msg):
            ops.rows_pool(a["y"], a["row_off"], a["lo"], a["hi"], out=a["out"])
    d = torch.zeros(4, 768, dtype=torch.bfloat16)
    for kw, msg in ((dict(dq=d.float()), "bfloat16"), (dict(dg=d[:, :512]), "768"),
                    (dict(idx=torch.tensor([0, 4], dtype=torch.int32)), "outside"),
                    (dict(idx=torch.tensor([-1], dtype=torch.int32)), "outside"),
                    (dict(idx=torch.tensor([0])), "int32")):
        a = dict(dq=d, dg=d, idx=None)
        a.update(kw)
        with pytest.raises(_lib.FpmError, match=msg):
            ops.desc_score(a["dq"], a["dg"], a["idx"])

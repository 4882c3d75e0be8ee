"""Enrolment from keypoints, host side (no GPU): ``ops.rows_pack`` on CPU tensors (the statement the kernel
is held to) and its refusals, the probe staging helper on numpy / tensor dicts, and the argument refusals
of ``enroll_keypoints`` / ``enroll_images`` / ``probe_graphs`` that need no device."""
import numpy as np
import pytest
import torch

import fpm
from fpm import _lib, gallery, ops, synth

PACK_NMAX = 40
PACK_NS = (1, 15, 16, 17, 33, 40, 0, 32)     # both sides of the 16-row band, an empty graph, a full graph


def special_block(rows, seed=9):
    """(rows, 768) fp32: random values, then in the first row +-0, subnormals, +-inf and values below, on
    (even and odd kept half) and above a bf16 rounding tie."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, 768, generator=g)
    bits = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x7F800000,
            0xFF800000, 0x3F807FFF, 0x3F808000, 0x3F808001, 0x3F817FFF, 0x3F818000, 0x3F818001, 0xBF808000,
            0xBF818000, 0x7F7FFFFF, 0x7F7F8000, 0x00007FFF]
    sp = torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32).view(torch.float32)
    x[0, :len(bits)] = sp
    x[rows - 1, 768 - len(bits):] = sp
    return x


def pack_case(ns=PACK_NS, nmax=PACK_NMAX):
    """Padded source (NaN in the padding rows), n, offsets and the statement of the pack."""
    B = len(ns)
    src = torch.full((B, nmax, 768), float("nan"))
    rows = special_block(sum(ns))
    n = torch.tensor(ns, dtype=torch.int32)
    off = torch.cat([torch.zeros(1, dtype=torch.int64), n.long().cumsum(0)])
    for b, k in enumerate(ns):
        src[b, :k] = rows[int(off[b]):int(off[b + 1])]
    want = torch.cat([src.view(B * nmax, 768)[b * nmax:b * nmax + k] for b, k in enumerate(ns)])
    assert torch.equal(want.view(torch.int32), rows.view(torch.int32))
    return src.view(B * nmax, 768), n, off, want


@pytest.mark.parametrize("which", ["out32", "out16", "both"])
def test_rows_pack_host(which):
    src, n, off, want = pack_case()
    total = int(off[-1])
    o32 = torch.full((total + 2, 768), float("nan")) if which != "out16" else None
    o16 = torch.full((total + 2, 768), float("nan"), dtype=torch.bfloat16) if which != "out32" else None
    got = ops.rows_pack(src, n, PACK_NMAX, off, out32=o32, out16=o16)
    assert got[0] is o32 and got[1] is o16
    if o32 is not None:
        assert torch.equal(o32[:total].view(torch.int32), want.view(torch.int32))
        assert bool(torch.isnan(o32[total:]).all())
    if o16 is not None:
        assert torch.equal(o16[:total].view(torch.int16), want.to(torch.bfloat16).view(torch.int16))
        assert bool(torch.isnan(o16[total:]).all())


def test_rows_pack_host_offset_base():
    """The offsets need not start at 0: a sub-batch packs into its place in a larger index."""
    src, n, off, want = pack_case()
    total = int(off[-1])
    out = torch.full((total + 7, 768), float("nan"))
    ops.rows_pack(src, n, PACK_NMAX, off + 5, out32=out)
    assert torch.equal(out[5:5 + total].view(torch.int32), want.view(torch.int32))
    assert bool(torch.isnan(out[:5]).all()) and bool(torch.isnan(out[5 + total:]).all())


def test_rows_pack_refusals(monkeypatch):
    def trap(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", trap)
    src, n, off, want = pack_case()
    total = int(off[-1])
    o32, o16 = torch.empty(total, 768), torch.empty(total, 768, dtype=torch.bfloat16)
    ops.rows_pack(src, n, PACK_NMAX, off, out32=o32, out16=o16)
    R = lambda m: pytest.raises(_lib.FpmError, match=m)
    with R("give out32, out16 or both"):
        ops.rows_pack(src, n, PACK_NMAX, off)
    with R("n must be a int32"):
        ops.rows_pack(src, n.long(), PACK_NMAX, off, out32=o32)
    with R("out_off must be a int64"):
        ops.rows_pack(src, n, PACK_NMAX, off.int(), out32=o32)
    with R("src must be contiguous fp32 rows"):
        ops.rows_pack(src.double(), n, PACK_NMAX, off, out32=o32)
    with R("out32 must be contiguous fp32 rows"):
        ops.rows_pack(src, n, PACK_NMAX, off, out32=o16)
    with R("out16 must be contiguous bf16 rows"):
        ops.rows_pack(src, n, PACK_NMAX, off, out16=o32)
    with R("out16 must be contiguous bf16 rows"):
        ops.rows_pack(src, n, PACK_NMAX, off, out16=o16.to(torch.float16))
    # non-contiguous inputs
    with R("src must be contiguous fp32 rows"):
        ops.rows_pack(torch.empty(src.shape[0], 1536)[:, ::2], n, PACK_NMAX, off, out32=o32)
    with R("out32 must be contiguous fp32 rows"):
        ops.rows_pack(src, n, PACK_NMAX, off, out32=torch.empty(total, 1536)[:, ::2])
    with R("n must be a contiguous 1-d"):
        ops.rows_pack(src, torch.stack([n, n], 1)[:, 0], PACK_NMAX, off, out32=o32)
    with R("out_off must be a contiguous 1-d"):
        ops.rows_pack(src, n, PACK_NMAX, torch.stack([off, off], 1)[:, 0], out32=o32)
    # counts and offsets
    big = n.clone()
    big[2] = PACK_NMAX + 1
    with R(r"n = 41 outside \[0, nmax = 40\]"):
        ops.rows_pack(src, big, PACK_NMAX, off, out32=o32)
    neg = n.clone()
    neg[2] = -1
    with R(r"n = -1 outside \[0, nmax = 40\]"):
        ops.rows_pack(src, neg, PACK_NMAX, off, out32=o32)
    bad = off.clone()
    bad[3] += 1
    with R("out_off must rise"):
        ops.rows_pack(src, n, PACK_NMAX, bad, out32=o32)
    with R("out_off must rise"):
        ops.rows_pack(src, n, PACK_NMAX, off - 1, out32=o32)
    with R("out_off must hold 9 offsets"):
        ops.rows_pack(src, n, PACK_NMAX, off[:-1], out32=o32)
    with R("host copies"):
        ops.rows_pack(src, n, PACK_NMAX, off, out32=o32, n_host=n[:-1])
    # outputs too small
    with R("out32 holds %d rows, the offsets end at %d" % (total - 1, total)):
        ops.rows_pack(src, n, PACK_NMAX, off, out32=o32[:-1])
    with R("out16 holds %d rows, the offsets end at %d" % (total - 1, total)):
        ops.rows_pack(src, n, PACK_NMAX, off, out32=o32, out16=o16[:-1])
    with R("out32 holds %d rows, the offsets end at %d" % (total, total + 1)):
        ops.rows_pack(src, n, PACK_NMAX, off + 1, out32=o32)
    with R("src holds 320 rows"):
        ops.rows_pack(src, n, PACK_NMAX + 1, off, out32=o32)
    # the grid's extent
    B = 65536
    with R("at most 65535 graphs"):
        ops.rows_pack(torch.empty(B, 768), torch.ones(B, dtype=torch.int32), 1, torch.arange(B + 1), out32=torch.empty(B, 768))


# ------------------------------------------------------------------------------------ probe helper
def test_probe_tensors_numpy_and_tensors():
    """numpy dicts (as ever), host-tensor dicts and dicts of tensors on the target device stage alike."""
    g = synth.make_graph(40, 2, 0, 23)
    as_t = {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    wide = dict(as_t, edge_index=as_t["edge_index"].long(), x=as_t["x"].double(), pseudo=as_t["pseudo"].double())
    ref = gallery._probe_tensors(g, "cpu")
    # what probe_batch / _ProbeSide staged from a numpy dict before the helper
    old = (int(g["n"]), torch.from_numpy(np.ascontiguousarray(np.asarray(g["x"], dtype=np.float32))),
           torch.from_numpy(np.asarray(g["edge_index"]).astype(np.int32)),
           torch.from_numpy(np.asarray(g["pseudo"], dtype=np.float32).reshape(-1, 2)),
           torch.from_numpy(np.asarray(g["w"], dtype=np.float32)))
    want_dt = (torch.float32, torch.int32, torch.float32, torch.float32)
    for got in (ref, gallery._probe_tensors(as_t, "cpu"), gallery._probe_tensors(wide, "cpu")):
        assert got[0] == old[0] == 23
        for a, b, dt in zip(got[1:], old[1:], want_dt):
            assert a.dtype == dt and a.shape == b.shape and torch.equal(a, b)
        assert got[1].is_contiguous() and tuple(got[2].shape)[0] == 2 and tuple(got[3].shape)[1] == 2
    # a tensor already on the device in the staged dtype is taken as it is
    fit = dict(as_t, x=as_t["x"].float(), edge_index=as_t["edge_index"].int(), pseudo=as_t["pseudo"].float(),
               w=as_t["w"].float())
    got = gallery._probe_tensors(fit, "cpu")
    for a, k in zip(got[1:], ("x", "edge_index", "pseudo", "w")):
        assert a.data_ptr() == fit[k].data_ptr(), k


# --------------------------------------------------------------------------------- argument refusals
@pytest.fixture(scope="module")
def net():
    return fpm.Net(regression=True, backbone=False).eval()


def _args(G=3, nmax=8):
    g = torch.Generator().manual_seed(1)
    return (torch.rand(G, nmax, 2, generator=g), torch.tensor([nmax, 5, 3][:G]), torch.randn(G, nmax, 768, generator=g),
            torch.rand(G, 512, generator=g))


def test_enroll_keypoints_refusals(net):
    P, n, x, w = _args()
    R = lambda m: pytest.raises(_lib.FpmError, match=m)
    net.train()
    try:
        with R("enroll_keypoints: inference only"):
            net.enroll_keypoints(P, n, x, w)
    finally:
        net.eval()
    with R("layout must be one of"):
        net.enroll_keypoints(P, n, x, w, layout="bf16")
    with R("sc_mode must be 'f32', or 'bf16' on a dtype='bf16' net"):
        net.enroll_keypoints(P, n, x, w, sc_mode="bf16")
    with R("sc_mode must be"):
        net.enroll_keypoints(P, n, x, w, sc_mode="f16")
    with R("empty gallery"):
        net.enroll_keypoints(P[:0], n[:0], x[:0], w[:0])
    with R(r"a graph of 9 keypoints; counts must lie in \[1, nmax = 8\]"):
        net.enroll_keypoints(P, torch.tensor([8, 9, 3]), x, w)
    with R(r"a graph of 0 keypoints; counts must lie in \[1, nmax = 8\]"):
        net.enroll_keypoints(P, torch.tensor([8, 0, 3]), x, w)
    with R("2 keypoint counts for 3 graphs"):
        net.enroll_keypoints(P, n[:2], x, w)
    with R(r"P must be \(G, nmax, 2\)"):
        net.enroll_keypoints(P.view(-1, 2), n, x, w)
    with R("x must be"):
        net.enroll_keypoints(P, n, x[:, :7], w)
    with R("x must be"):
        net.enroll_keypoints(P, n, x[..., :767], w)
    with R("w must be"):
        net.enroll_keypoints(P, n, x, w[:2])
    # arrays are taken like tensors: the same refusal from numpy inputs
    with R("counts must lie in"):
        net.enroll_keypoints(P.numpy(), [8, 9, 3], x.view(-1, 768).numpy(), w.numpy())


def test_enroll_images_and_probe_graphs_refusals(net):
    P, n, x, w = _args()
    img = torch.zeros(3, 3, 16, 16)
    with pytest.raises(NotImplementedError, match="image input needs the backbone"):
        net.enroll_images(img, P, n)
    with pytest.raises(NotImplementedError, match="image input needs the backbone"):
        net.probe_graphs(P, n, images=img)
    R = lambda m: pytest.raises(_lib.FpmError, match=m)
    with R("give the features x and w, or images"):
        net.probe_graphs(P, n)
    with R("give the features x and w, or images"):
        net.probe_graphs(P, n, x=x)
    with R("give the features x and w, or images"):
        net.probe_graphs(P, n, x=x, w=w, images=img)
    with R(r"probe_graphs: a graph of 9 keypoints; counts must lie in \[1, nmax = 8\]"):
        net.probe_graphs(P, [8, 9, 3], x=x, w=w)
    with R("probe_graphs: x must be"):
        net.probe_graphs(P, n, x=x[:2], w=w)

"""The GNN layer's resident kernel (boxes of at most 256 keypoints: 64 registers, 72-B LDS node
rows, eight workgroups per CU; ``gnn_form`` 1) against the kernel it replaced there (``gnn_form`` 0),
bit for bit, on random X and random weights over hand-built graphs.

The graphs are built on the CPU (``gnn_ref._graphs``) so that the shapes the kernel can go wrong at are
certain to occur: graph-2 neighbour lists of every length 0..7 (every remainder of the batches of
rows phase 1 keeps in flight), a graph-1 node of degree 0 and one of degree 12, pairs shorter than
the box (the diagonal term's ``p < n1 * n2`` edge, padded nodes with empty lists), boxes that are no
multiple of the wave, and fewer pairs than the grid's padding to 8."""
import pytest
import torch

from fpm import _lib, ops
from gnn_ref import SHAPES, _graphs

DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fixture_has_every_list_length(shape):
    """CPU: every pair's graph 2 holds lists of every length 0..7, its graph 1 a node of degree 0 and
    one of degree 12, padded nodes have empty lists, and the CSR is the non-decreasing batch CSR."""
    n1max, n2max, n1s, n2s = SHAPES[shape]
    (ptr1, nbr1, ptr2, nbr2, _, _), l1, l2 = _graphs(shape)
    for b, (n1, n2) in enumerate(zip(n1s, n2s)):
        assert {len(r) for r in l2[b][:n2]} == set(range(8))
        assert all(len(r) == 0 for r in l2[b][n2:]) and all(len(r) == 0 for r in l1[b][n1:])
        d1 = [len(r) for r in l1[b][:n1]]
        assert 0 in d1 and 12 in d1
        assert all(0 <= a < n1 for r in l1[b] for a in r) and all(0 <= e < n2 for r in l2[b] for e in r)
    for ptr, nbr, nmax in ((ptr1, nbr1, n1max), (ptr2, nbr2, n2max)):
        assert ptr.numel() == len(n1s) * nmax + 1 and int(ptr[0]) == 0
        assert bool((ptr[1:] >= ptr[:-1]).all()) and int(ptr[-1]) == nbr.numel() - 1
    # the lengths as the kernel reads them
    lens = (ptr2[1:] - ptr2[:-1]).view(len(n2s), n2max)
    for b in range(len(n2s)):
        assert set(lens[b].tolist()) == set(range(8))


def _run(form, C, shape, last, ord_on):
    n1max, n2max, n1s, n2s = SHAPES[shape]
    B = len(n1s)
    cpu, _, _ = _graphs(shape)
    ptr1, nbr1, ptr2, nbr2, n1, n2 = (t.to(DEV) for t in cpu)
    g = torch.Generator().manual_seed(C * 100 + n1max + 3 * n2max + last)
    X = torch.randn(B, C, n2max, n1max, generator=g).to(DEV)
    W = (torch.randn(_lib.load().fpm_gnn_param_count(C), generator=g) * 0.3).to(DEV)
    cls_w = torch.randn(17, generator=g).to(DEV) if last else None
    ord2 = None
    if ord_on:
        ord2 = torch.stack([torch.randperm(n2max, generator=g) for _ in range(B)]).to(torch.int32).to(DEV)
    # one guard pair behind the B real ones: the grid pads the pairs to 8, and pairs B..7 write nothing
    Xo = torch.full((B + 1, 17, n2max, n1max), 5.0, device=DEV)
    z = torch.full((B + 1, n2max, n1max), 5.0, device=DEV)
    vp = torch.full((B + 1, n2max, n1max), 5.0, device=DEV) if last else None
    prev = ops.set_tuning("gnn_form", form)
    try:
        ops.gnn_layer(X, C, B, n1max, n2max, (ptr1.data_ptr(), nbr1.data_ptr()), (ptr2.data_ptr(), nbr2.data_ptr()),
                      n1, n2, W, Xo[:B], z[:B], vpart=vp[:B] if last else None, cls_w=cls_w, ord2=ord2)
        torch.cuda.synchronize()
    finally:
        ops.set_tuning("gnn_form", prev)
    return Xo, z, vp


@pytest.mark.gpu
@pytest.mark.parametrize("ord_on", [False, True], ids=["id", "ord2"])
@pytest.mark.parametrize("last", [False, True], ids=["plain", "last"])
@pytest.mark.parametrize("C", [1, 17])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_resident_form_bit_identical(shape, C, last, ord_on):
    """gnn_form 1 against gnn_form 0: every written array equal bit for bit, what a form leaves alone
    (channel 16, the outputs of the other layer form, the guard pair) left alone by both."""
    B = len(SHAPES[shape][2])
    new = _run(1, C, shape, last, ord_on)
    old = _run(0, C, shape, last, ord_on)
    for name, a, r in zip(("Xout", "z", "vpart"), new, old):
        if a is None:
            assert r is None
            continue
        assert bool(torch.isfinite(r).all()), name
        assert torch.equal(a, r), name
        assert bool((a[B] == 5.0).all()), name + ": guard pair written"
    Xo, z, vp = new
    assert bool((Xo[:B, 16] == 5.0).all())
    assert not bool((z[:B] == 5.0).all())
    if last:
        assert bool((Xo == 5.0).all()) and not bool((vp[:B] == 5.0).all())
    else:
        assert not bool((Xo[:B, :16] == 5.0).any())


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 17])
def test_resident_form_eight_workgroups_per_cu(C):
    """No kernel runs: the occupancy query reports at least 8 workgroups of 256 threads per CU for
    the resident kernel at the full box's LDS size (18 KiB at C = 17), and the query answers for
    the other form and for a box over 256 too."""
    prev = ops.set_tuning("gnn_form", 1)
    try:
        assert ops.gnn_resident_blocks(C, 256) >= 8
        assert ops.gnn_resident_blocks(C, 512) >= 1
        ops.set_tuning("gnn_form", 0)
        assert ops.gnn_resident_blocks(C, 256) >= 1
    finally:
        ops.set_tuning("gnn_form", prev)

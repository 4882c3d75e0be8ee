"""Where the stored fields of a ``GalleryIndex`` live on the GPU, after every operation that re-makes them: on the
index device, in pinned host memory or in plain host memory, as the class docstring states (the CPU census,
``test_index_fields_cpu.py``, sees the values but not the placement).  The shape is tiny on purpose."""
import pytest
import torch

from fpm import params
from fpm.gallery import GalleryIndex
from test_enroll_keypoints_gpu import DEV, _keypoint_set, _net

pytestmark = pytest.mark.gpu

LAYOUTS = ("f32", "f32+bf16", "bf16+host", "fp8+host")
ROW_FIELDS = {"f32": ("y",), "f32+bf16": ("y", "y16"), "bf16+host": ("y", "y16"), "fp8+host": ("y", "y8", "s8")}
DEVICE = ("P", "src", "dst", "pseudo", "w", "desc", "row_off")          # whatever the layout
HOST = ("n", "edge_off", "row_off_host", "subject")
ABSENT = {"f32": ("y16", "y8", "s8"), "f32+bf16": ("y8", "s8"), "bf16+host": ("y8", "s8"), "fp8+host": ("y16",)}
NS = [8, 5, 7, 8, 3, 6]
SUBJECTS = [4, 4, 0, 2, 0, 2]


def placed(idx, layout, what):
    host_rows = layout in ("bf16+host", "fp8+host")
    assert idx.layout == layout and idx.device == DEV, what
    for k in ROW_FIELDS[layout] + DEVICE + HOST:
        assert isinstance(getattr(idx, k), torch.Tensor), (what, k)
    for k in ABSENT[layout]:
        assert getattr(idx, k) is None, (what, k)
    for k in ROW_FIELDS[layout][1:] + DEVICE + (() if host_rows else ("y",)):
        assert getattr(idx, k).device == DEV, (what, k)
    if host_rows:
        assert not idx.y.is_cuda and idx.y.is_pinned(), what
    for k in HOST:
        t = getattr(idx, k)
        assert not t.is_cuda and not t.is_pinned(), (what, k)
    assert torch.equal(idx.row_off.cpu(), idx.row_off_host), what


def pointers(idx, layout):
    return {k: getattr(idx, k).data_ptr() for k in ROW_FIELDS[layout]}


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fields_live_where_the_docstring_says(layout, tmp_path):
    net = _net(params.init_params(7), "bf16")
    P, n, x, w = (t.to(DEV) for t in _keypoint_set(NS, 21))
    idx = net.enroll_keypoints(P, n, x, w, batch=4, layout=layout, subjects=SUBJECTS, capacity=(8, 64),
                               descriptors=True)
    placed(idx, layout, "enroll_keypoints(capacity=)")
    assert idx.capacity == (8, 64, 6 * 64) and idx.used[:2] == (6, sum(NS))
    first = pointers(idx, layout)
    assert first == {k: idx._store[k].data_ptr() for k in first}                 # prefix views of the storage
    roomy = idx.reserve(10, 80)
    placed(roomy, layout, "reserve")
    placed(idx, layout, "reserve left its parent alone")
    assert pointers(idx, layout) == first                                       # ... and where it was
    assert all(pointers(roomy, layout)[k] != first[k] for k in first)            # storage of its own
    at = pointers(roomy, layout)
    roomy.remove([1, 4])
    assert roomy.compact().tolist() == [0, -1, 1, 2, -1, 3]
    placed(roomy, layout, "remove, compact")
    assert pointers(roomy, layout) == at and roomy.capacity[:2] == (10, 80)      # inside the same storage
    part = roomy.slice(torch.tensor([0, 2]), device=DEV)
    placed(part, layout, "slice(device=)")
    assert part.capacity is None and all(pointers(part, layout)[k] != at[k] for k in at)
    roomy.save(tmp_path / "index.pt")
    back = GalleryIndex.load(tmp_path / "index.pt", DEV, capacity=(8, 64))
    placed(back, layout, "save, load(capacity=)")
    assert back.capacity == (8, 64, 6 * 64) and back.used == roomy.used
    assert pointers(back, layout) == {k: back._store[k].data_ptr() for k in at}
    for k in ROW_FIELDS[layout] + ("P", "src", "dst", "pseudo", "w", "desc", "n", "edge_off", "subject"):
        a, b = getattr(back, k).cpu(), getattr(roomy, k).cpu()
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), k

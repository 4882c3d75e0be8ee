"""bench.py --dump-outputs: the writer's host logic (CPU): every array of a result dict lands as
float32 / float64 ``<name>.npy``, outputs over their share of the budget are cut to one fixed, seeded
sample of whole pairs shared by all of them, the directory stays under the 64 MB limit, and two calls
write the same bytes."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def _result(B, n):
    g = torch.Generator().manual_seed(5)
    return {"s": torch.rand(B, n, n, generator=g), "ds_mat": torch.rand(B, n, n, generator=g),
            "perm_mat": (torch.rand(B, n, n, generator=g) > 0.9).float(),
            "k_prob": torch.rand(B, generator=g), "sk_steps": torch.arange(B, dtype=torch.int32),
            "half": torch.rand(B, generator=g).bfloat16(), "ks_loss": None, "scalar": torch.tensor(1.5)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_written_whole(tmp_path):
    res = _result(6, 8)
    shapes = bench.dump_outputs(res, str(tmp_path / "a"))
    got = _load(str(tmp_path / "a"))
    assert set(got) == {k for k, v in res.items() if v is not None} and set(shapes) == set(got)
    for k, a in got.items():
        assert a.dtype == (np.float64 if k == "sk_steps" else np.float32), k
        np.testing.assert_array_equal(a, res[k].double().numpy().astype(a.dtype))
        assert list(a.shape) == shapes[k]


def test_large_outputs_sampled_by_pair(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 6 << 20)          # 3 large outputs -> 2 MiB each
    B, n = 40, 128                                               # 64 KiB per pair, 2.5 MiB per output
    res = _result(B, n)
    bench.dump_outputs(res, str(tmp_path / "a"), seed=3)
    bench.dump_outputs(res, str(tmp_path / "b"), seed=3)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    idx = a["sample_pairs"].astype(np.int64)
    assert len(idx) == 32 and len(set(idx)) == 32 and (np.diff(idx) > 0).all() and idx.max() < B
    for k in ("s", "ds_mat", "perm_mat"):
        np.testing.assert_array_equal(a[k], res[k].numpy()[idx])
    np.testing.assert_array_equal(a["k_prob"], res["k_prob"].numpy())
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    size = sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a")))
    assert size <= (6 << 20) + 4096 * len(a)


def test_default_budget_under_limit():
    assert bench.DUMP_BYTES + (8 << 20) <= 64 << 20        # room for the small per-pair vectors

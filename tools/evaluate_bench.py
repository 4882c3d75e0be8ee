"""Times ``ops.mate_rank``, ``ops.score_census`` and ``ops.score_select`` against the plain-torch route on the same
device: ``torch.sort`` per row for the mate's rank, ``torch.bucketize`` + ``torch.bincount`` for the census.

    python tools/evaluate_bench.py [--out profiles/evaluate.json] [--shapes 16x1048576,16384x16384]

Device events, 1 warm-up and 7 runs per figure: median (min - max) in milliseconds.  The bytes a kernel must read
are computed from the shape (scores once or twice, plus the labels); "GB/s" is those bytes over the median.
Shared labels, one genuine column per row, every other column an impostor; the results of the two routes
are compared before anything is timed.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fpm import ops  # noqa: E402

DEV = torch.device("cuda", 0)


def timed(fn, warmup=1, runs=7):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def case(P, G, T):
    g = torch.Generator(device=DEV).manual_seed(P + G)
    s = torch.randn(P, G, device=DEV, generator=g)
    mate = torch.randint(0, G, (P,), device=DEV, generator=g)
    col = torch.arange(G, dtype=torch.int32, device=DEV)         # shared labels: entry j is subject j
    s[torch.arange(P, device=DEV), mate] += 2.0
    row = mate.to(torch.int32)
    edges = torch.linspace(-6.0, 8.0, T, device=DEV)
    return s, row, col, mate, edges


def torch_rank(s, mate):
    order = torch.sort(s, dim=1, descending=True, stable=True).indices
    return (order == mate.view(-1, 1)).to(torch.int8).argmax(1)


def torch_census(s, row, col, edges):
    b = torch.bucketize(s, edges, right=True)
    n = int(edges.numel()) + 1
    gen = col.view(1, -1) == row.view(-1, 1)
    return torch.bincount(b[gen], minlength=n), torch.bincount(b[~gen], minlength=n)


def bench(P, G, T):
    s, row, col, mate, edges = case(P, G, T)
    mc, _, mr = ops.mate_rank(s, row, col)
    assert torch.equal(mc.long(), mate) and torch.equal(mr.long(), torch_rank(s, mate))
    gen, imp, skipped = ops.score_census(s, row, col, edges)
    tg, ti = torch_census(s, row, col, edges)
    assert torch.equal(gen, tg) and torch.equal(imp, ti) and int(skipped.sum()) == 0
    k = max(1, P * G // 1000)
    v, n = ops.score_select(s, row, col, "impostor", k)
    assert n == P * (G - 1) and float(v) == float(torch.topk(s[col.view(1, -1) != row.view(-1, 1)], k).values[-1])
    score_b, lab_b = 4 * P * G, 4 * G
    out = dict(P=P, G=G, T=T, k=k)
    for name, fn, nbytes in (
            ("mate_rank", lambda: ops.mate_rank(s, row, col), 2 * (score_b + lab_b)),
            ("torch_sort_rank", lambda: torch_rank(s, mate), None),
            ("score_census", lambda: ops.score_census(s, row, col, edges), score_b + lab_b),
            ("torch_bucketize_bincount", lambda: torch_census(s, row, col, edges), None),
            ("score_select", lambda: ops.score_select(s, row, col, "impostor", k), 3 * (score_b + lab_b))):
        r = timed(fn)
        if nbytes:
            r["bytes"] = nbytes
            r["GBps"] = nbytes / r["median_ms"] / 1e6
        out[name] = r
        print("%-26s %6d x %-8d %9.3f ms (%.3f - %.3f)%s" % (
            name, P, G, r["median_ms"], r["min_ms"], r["max_ms"], "  %.0f GB/s" % r["GBps"] if nbytes else ""), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="16x1048576,16384x16384")
    ap.add_argument("--edges", type=int, default=1023)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), warmup=1, runs=7, labels="shared (G,) int32",
               cases=[bench(*[int(v) for v in sh.split("x")], a.edges) for sh in a.shapes.split(",")])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

"""Enrolment: ``Net.enroll`` on host graph dicts against ``Net.enroll_keypoints`` on device tensors of the
same graphs, and the ragged pack kernel (``ops.rows_pack``) alone.  GPU.

    python tools/enroll_bench.py [--gallery 1024] [--n 128] [--batch 256] [--reps 7]
                                 [--layouts f32,bf16+host] [--peak-gallery 8192]
                                 [--out profiles/enroll_keypoints.json]

Shape: 1024 graphs of up to 128 keypoints (random distinct points, Delaunay; counts in [96, 128], every
sub-batch padded to 128), bf16 net.  The graphs are built once on the device and exported to host dicts;
both sides then enrol the same graphs in one process, per layout: one warm-up, ``--reps`` timed runs each,
HIP events around each run plus wall time; median (min - max) and the A/B verdict of DESIGN 5 with
``enroll`` as the baseline (the candidate's median against the baseline's best run less the baseline's own
spread).  ``enroll`` is timed from the host dicts (it pads and uploads them: that is the path),
``enroll_keypoints`` from P / x / w resident on the device (it builds the graphs: that is the path); the
two indexes are compared field by field once.  Next to each: ``torch.cuda.max_memory_allocated`` over one
run (the peak above what was resident before the call) and the index's ``nbytes()``.

``--peak-gallery G2`` (0: skip): the same memory figures, "f32" layout, for a gallery of G2 graphs, one run
of each side, untimed: at 1024 graphs one sub-batch's SplineConv workspace is several times the index, so
how the index itself is assembled shows only in a larger gallery.

The pack kernel alone: one sub-batch's padded rows into fp32, bf16 and both, against the torch statements
it replaces on the same rows (``y[keep]``; ``y[keep]`` and ``cast_bf16`` of it); ``PACK_INNER`` launches
back to back per timed run, bytes read and written per second.  Writes one JSON file.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FIELDS = ("y", "y16", "row_off", "n", "src", "dst", "pseudo", "edge_off", "w", "P")
PACK_INNER = 50


def _timed(fn, reps, inner=1):
    """[(GPU ms between events around fn, wall ms)] of ``reps`` runs; a run is ``inner`` calls back to back
    (a kernel of tens of microseconds is timed over many launches), the times per call."""
    import torch
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append((e0.elapsed_time(e1) / inner, (time.perf_counter() - t) * 1e3 / inner))
    return out


def _summary(samples, digits=3):
    ev = sorted(s[0] for s in samples)
    wall = sorted(s[1] for s in samples)
    r = lambda v: round(v, digits)
    return dict(in_order_ms=[r(s[0]) for s in samples], median_ms=r(statistics.median(ev)), min_ms=r(ev[0]),
                max_ms=r(ev[-1]), wall_median_ms=r(statistics.median(wall)), wall_min_ms=r(wall[0]),
                wall_max_ms=r(wall[-1]))


def _verdict(o, c, key="", digits=3):
    # the project's A/B rule: the candidate's median against the baseline's best run less its spread
    med, lo, hi = key + "median_ms", key + "min_ms", key + "max_ms"
    faster = o[lo] - (o[hi] - o[lo]) - c[med]
    slower = c[lo] - (c[hi] - c[lo]) - o[med]
    return dict(speedup_median=round(o[med] / c[med], 3), faster_margin_ms=round(faster, digits),
                slower_margin_ms=round(slower, digits),
                verdict="faster" if faster > 0 else "slower" if slower > 0 else "within spread")


def _peak(fn, dev):
    """(bytes allocated before the call, the call's peak above that, what the result holds) of one run."""
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    index = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    return dict(resident_before_bytes=int(before), peak_bytes=int(peak), index_nbytes=int(index.nbytes()),
                index_host_nbytes=int(index.host_nbytes()), peak_over_index=round(peak / index.nbytes(), 3))


def _graphs(G, n, batch, dev, seed):
    """G random keypoint graphs of [3n/4, n] keypoints (every sub-batch pads to n) -> (counts, P, x, w on
    the host, the same graphs as host dicts, edges in all)."""
    import numpy as np
    import torch
    from fpm import graphs
    g = torch.Generator().manual_seed(seed)
    cnt = torch.randint(n * 3 // 4, n + 1, (G,), generator=g, dtype=torch.int32)
    cnt[::batch] = n
    keep = (torch.arange(n)[None, :] < cnt.view(-1, 1))[..., None]
    P = torch.rand(G, n, 2, generator=g) * torch.tensor([320.0, 240.0]) * keep
    x = torch.randn(G, n, 768, generator=g) * keep
    w = torch.rand(G, 512, generator=g)
    gb = graphs.build_graph_batch(P.to(dev), cnt)
    eo = gb.edge_off_host.tolist()
    src, dst, ps = (gb.src % n).cpu().numpy(), (gb.dst % n).cpu().numpy(), gb.pseudo.cpu().numpy()
    dicts = [dict(n=int(k), x=x[i, :k].numpy(), w=w[i].numpy(), P=P[i, :k].numpy(),
                  edge_index=np.stack([src[eo[i]:eo[i + 1]], dst[eo[i]:eo[i + 1]]]), pseudo=ps[eo[i]:eo[i + 1]])
             for i, k in enumerate(cnt.tolist())]
    return cnt, P, x, w, dicts, int(eo[-1])


def _pack_alone(n, batch, reps, dev):
    import torch
    from fpm import ops
    g = torch.Generator().manual_seed(2)
    cnt = torch.randint(n * 3 // 4, n + 1, (batch,), generator=g, dtype=torch.int32)
    cnt[0] = n
    off = torch.cat([torch.zeros(1, dtype=torch.int64), cnt.long().cumsum(0)])
    rows = int(off[-1])
    src = torch.randn(batch * n, 768, device=dev)
    cnt_d, off_d = cnt.to(dev), off.to(dev)
    o32 = torch.empty(rows, 768, device=dev)
    o16 = torch.empty(rows, 768, device=dev, dtype=torch.bfloat16)
    keep = (torch.arange(n, device=dev)[None, :] < cnt_d.view(-1, 1)).reshape(-1)

    def torch_f32():                     # what enroll runs per sub-batch for the "f32" layout
        return src[keep]

    def torch_both():                    # ... and for the layouts with a bf16 copy (the host copy not included)
        ops.cast_bf16(src[keep], out=o16)

    pack = lambda **kw: (lambda: ops.rows_pack(src, cnt_d, n, off_d, n_host=cnt, out_off_host=off, **kw))
    res = dict(graphs=batch, nmax=n, rows=rows, launches_per_run=PACK_INNER,
               note="src + outputs of one sub-batch (under 256 MB) can stay in the Infinity Cache between launches")
    for name, fn, wbytes in (("out32", pack(out32=o32), 4), ("out16", pack(out16=o16), 2),
                             ("both", pack(out32=o32, out16=o16), 6), ("torch_index", torch_f32, None),
                             ("torch_index_cast", torch_both, None)):
        fn()
        s = _summary(_timed(fn, reps, PACK_INNER), 4)
        if wbytes:
            s["bytes"] = rows * 768 * (4 + wbytes)
            s["GBps"] = round(s["bytes"] / s["median_ms"] / 1e6, 1)
        res[name] = s
    res["ab_out32_vs_torch_index"] = _verdict(res["torch_index"], res["out32"], digits=4)
    res["ab_both_vs_torch_index_cast"] = _verdict(res["torch_index_cast"], res["both"], digits=4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=1024)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--layouts", default="f32,bf16+host")
    ap.add_argument("--peak-gallery", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "enroll_keypoints.json"))
    args = ap.parse_args()
    import torch
    import fpm
    from fpm import params

    dev = torch.device("cuda", 0)
    G, n = args.gallery, args.n
    net = fpm.Net(regression=True, backbone=False, dtype="bf16")
    net.load_state_dict(params.init_params(7))
    cnt, P, x, w, dicts, edges = _graphs(G, n, args.batch, dev, 1)
    Pd, xd, wd = P.to(dev), x.to(dev), w.to(dev)
    res = dict(tool="tools/enroll_bench.py --gallery %d --n %d --batch %d --reps %d --layouts %s --peak-gallery %d"
                    % (G, n, args.batch, args.reps, args.layouts, args.peak_gallery), gallery=G, n=n,
               batch=args.batch, keypoints=int(cnt.sum()), edges=edges, dtype="bf16", reps=args.reps,
               method="1 warm-up, `reps` runs each, HIP events around each run and wall time, median and min-max; "
                      "both sides in one process on the same graphs; enroll from host dicts, enroll_keypoints from "
                      "device tensors; verdict by the A/B rule with enroll as the baseline",
               device=torch.cuda.get_device_name(dev), layouts={})
    for lay in args.layouts.split(","):
        old = lambda: net.enroll(dicts, dev, batch=args.batch, layout=lay)
        new = lambda: net.enroll_keypoints(Pd, cnt, xd, wd, batch=args.batch, layout=lay)
        a, b = old(), new()                                      # the warm-up, and the comparison
        same = all((getattr(a, k) is None and getattr(b, k) is None) or torch.equal(getattr(a, k), getattr(b, k))
                   for k in FIELDS)
        del a, b
        r = dict(same_index=bool(same))
        r["enroll"] = _summary(_timed(old, args.reps))
        r["enroll_keypoints"] = _summary(_timed(new, args.reps))
        r["ab_event"] = _verdict(r["enroll"], r["enroll_keypoints"])
        r["ab_wall"] = _verdict(r["enroll"], r["enroll_keypoints"], "wall_")
        r["enroll"]["memory"] = _peak(old, dev)
        r["enroll_keypoints"]["memory"] = _peak(new, dev)
        res["layouts"][lay] = r
        print("ENROLL_BENCH %s %s" % (lay, json.dumps(r)), flush=True)
    res["rows_pack_alone"] = _pack_alone(n, args.batch, args.reps, dev)
    print("ENROLL_BENCH rows_pack %s" % json.dumps(res["rows_pack_alone"]), flush=True)
    if args.peak_gallery:
        del Pd, xd, wd, dicts, P, x, w
        G2 = args.peak_gallery
        cnt, P, x, w, dicts, edges = _graphs(G2, n, args.batch, dev, 3)
        Pd, xd, wd = P.to(dev), x.to(dev), w.to(dev)
        r = dict(gallery=G2, keypoints=int(cnt.sum()), layout="f32", runs=1)
        r["enroll"] = _peak(lambda: net.enroll(dicts, dev, batch=args.batch), dev)
        r["enroll_keypoints"] = _peak(lambda: net.enroll_keypoints(Pd, cnt, xd, wd, batch=args.batch), dev)
        res["peak_large_gallery"] = r
        print("ENROLL_BENCH peak %s" % json.dumps(r), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

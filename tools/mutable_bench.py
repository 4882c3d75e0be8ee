"""Mutable gallery index: what an append into reserved space costs next to enrolling the same graphs alone,
and how fast ``GalleryIndex.compact`` moves rows, next to the pack kernel's rate.  GPU.

    python tools/mutable_bench.py [--gallery 1024] [--append 256] [--n 128] [--batch 256] [--reps 7]
                                  [--compact-gallery 4096] [--layouts f32,f32+bf16,bf16+host]
                                  [--out profiles/mutable_index.json]

Append: an index of ``--gallery`` graphs of up to ``--n`` keypoints (``tools/enroll_bench.py``'s graphs, bf16
net) with room for ``--append`` more; ``Net.enroll_keypoints_into`` of those from device tensors against
``Net.enroll_keypoints`` of the same graphs alone (the path a caller without a mutable index re-runs for the
whole gallery).  Every timed append goes into a fresh ``reserve`` of the base index (made outside the timed
region), and every timed standalone run follows the same ``reserve``, so that both sides start from the same
cache state (the standalone runs back to back are listed too); 1 warm-up, ``--reps`` runs, HIP events and wall
time, the A/B rule of DESIGN 5 with the standalone enrolment as the baseline.

Compaction: a synthetic index of ``--compact-gallery`` entries of ``--n`` rows (random rows; compaction does
not look at them), every fourth entry removed, ``compact()`` with the default stage, per layout: wall time
(it ends with the host tables, so wall is the figure), the rows moved, and bytes read plus written per second
over the row bytes of the layout -- beside ``ops.rows_pack`` alone from the same process.  Writes one JSON file.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from enroll_bench import _graphs, _pack_alone, _summary, _timed, _verdict  # noqa: E402

ROW_BYTES = {"f32": 4 * 768, "f32+bf16": 6 * 768, "bf16+host": 2 * 768}      # the rows ops.rows_move carries


def _synthetic(G, n, layout, dev):
    import torch
    from fpm.gallery import GalleryIndex, _host_rows
    rows = G * n
    y = torch.randn(rows, 768, device=dev)
    y16 = None if layout == "f32" else y.to(torch.bfloat16)
    if layout == "bf16+host":
        y = _host_rows((rows, 768), dev).copy_(y)
    cnt = torch.full((G,), n, dtype=torch.int32)
    off = torch.arange(G + 1, dtype=torch.int64) * n
    z = torch.zeros(G * 6, dtype=torch.int32, device=dev)
    return GalleryIndex(y, off.to(dev), cnt, z, z.clone(), torch.zeros(G * 6, 2, device=dev),
                        torch.arange(G + 1, dtype=torch.int64) * 6, torch.zeros(G, 512, device=dev),
                        torch.zeros(rows, 2, device=dev), "bf16", 0, "bench", y16=y16, layout=layout)


def _compact(G, n, layout, reps, dev):
    import torch
    base = _synthetic(G, n, layout, dev)
    gone = list(range(1, G, 4))
    walls, last = [], None
    for rep in range(reps + 1):
        idx = base.reserve(*base.used)
        idx.remove(gone)
        torch.cuda.synchronize()
        t = time.perf_counter()
        idx.compact()
        torch.cuda.synchronize()
        if rep:                                                  # the first run is the warm-up
            walls.append((time.perf_counter() - t) * 1e3)
        last = idx.last_compact
        del idx
    med = statistics.median(walls)
    moved = last["rows"] * ROW_BYTES[layout] * 2
    r = dict(entries=G, rows=G * n, removed=len(gone), routes=last, wall_ms=[round(w, 3) for w in walls],
             wall_median_ms=round(med, 3), device_row_bytes_read_and_written=moved,
             GBps=round(moved / med / 1e6, 1))
    if layout == "bf16+host":
        r["host_row_bytes_moved"] = last["rows"] * 4 * 768 * 2
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=1024)
    ap.add_argument("--append", type=int, default=256)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--compact-gallery", type=int, default=4096)
    ap.add_argument("--layouts", default="f32,f32+bf16,bf16+host")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mutable_index.json"))
    args = ap.parse_args()
    import torch
    import fpm
    from fpm import params

    dev = torch.device("cuda", 0)
    G, A, n = args.gallery, args.append, args.n
    net = fpm.Net(regression=True, backbone=False, dtype="bf16")
    net.load_state_dict(params.init_params(7))
    cnt, P, x, w, _, _ = _graphs(G + A, n, args.batch, dev, 1)
    Pd, xd, wd = P.to(dev), x.to(dev), w.to(dev)
    res = dict(tool="tools/mutable_bench.py --gallery %d --append %d --n %d --batch %d --reps %d --compact-gallery %d "
                    "--layouts %s" % (G, A, n, args.batch, args.reps, args.compact_gallery, args.layouts),
               device=torch.cuda.get_device_name(dev), dtype="bf16", reps=args.reps, append={}, compact={},
               method="append: 1 warm-up, `reps` runs each, HIP events and wall time, every run of either side after "
                      "a fresh reserve() of the base index, the append into it; verdict by the A/B rule with the "
                      "standalone enrolment as the baseline.  compact: wall time of compact() after removing every fourth entry, 1 warm-up")
    for lay in args.layouts.split(","):
        base = net.enroll_keypoints(Pd[:G], cnt[:G], xd[:G], wd[:G], batch=args.batch, layout=lay)
        rows, edges = int(cnt.sum()), int(base.edge_off[-1]) * (G + A) // G + 4096
        alone = lambda: net.enroll_keypoints(Pd[G:], cnt[G:], xd[G:], wd[G:], batch=args.batch, layout=lay)
        fresh = []

        def into():
            return net.enroll_keypoints_into(fresh.pop(), Pd[G:], cnt[G:], xd[G:], wd[G:], batch=args.batch)

        def timed_after_reserve(fn, reps):
            # both sides run after the same reserve() of the base index (its copies pass through the caches that
            # back-to-back runs of one side alone would keep warm)
            out = []
            for _ in range(reps):
                fresh.append(base.reserve(G + A, rows, edges))
                if fn is alone:
                    fresh.pop()
                out += _timed(fn, 1)
            return out

        ref = alone()
        fresh.append(base.reserve(G + A, rows, edges))
        idx = fresh[0]
        new = into()
        same = torch.equal(idx.y[int(idx.row_off_host[G]):].cpu(), ref.y.cpu()) and new.tolist() == list(range(G, G + A))
        del idx, ref
        r = dict(same_rows=bool(same), gallery=G, appended=A)
        r["enroll_keypoints_alone_back_to_back"] = _summary(_timed(alone, args.reps))
        r["enroll_keypoints_alone"] = _summary(timed_after_reserve(alone, args.reps))
        r["enroll_keypoints_into"] = _summary(timed_after_reserve(into, args.reps))
        r["ab_event"] = _verdict(r["enroll_keypoints_alone"], r["enroll_keypoints_into"])
        r["ab_wall"] = _verdict(r["enroll_keypoints_alone"], r["enroll_keypoints_into"], "wall_")
        r["into_over_alone_median"] = round(r["enroll_keypoints_into"]["median_ms"] /
                                            r["enroll_keypoints_alone"]["median_ms"], 4)
        r["into_over_alone_wall_median"] = round(r["enroll_keypoints_into"]["wall_median_ms"] /
                                                 r["enroll_keypoints_alone"]["wall_median_ms"], 4)
        res["append"][lay] = r
        print("MUTABLE_BENCH append %s %s" % (lay, json.dumps(r)), flush=True)
        del base
    del Pd, xd, wd, P, x, w
    torch.cuda.empty_cache()
    for lay in args.layouts.split(","):
        res["compact"][lay] = _compact(args.compact_gallery, n, lay, min(args.reps, 5), dev)
        print("MUTABLE_BENCH compact %s %s" % (lay, json.dumps(res["compact"][lay])), flush=True)
        torch.cuda.empty_cache()
    res["rows_pack_alone"] = _pack_alone(n, args.batch, args.reps, dev)
    print("MUTABLE_BENCH rows_pack %s" % json.dumps(res["rows_pack_alone"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

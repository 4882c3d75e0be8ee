"""Gallery over several GPUs: what the merge kernel costs alone, what a sharded query costs over the one-index
query on one GPU (overhead only: the shards share the device), and whether the unchanged one-index call kept
its time.  Not part of ``bench.py``; nothing here is asserted anywhere.

    python tools/sharded_gallery_bench.py [--out FILE] [--parent TREE] [--rounds N] [--galleries 1024,16384]

Writes a text report (default ``profiles/r11_sharded_gallery.txt``):

  kernel    ``fpm_topk_merge`` (the C-ABI entry on preallocated outputs) and ``ops.topk_merge`` (the wrapper with its
            checks and allocations) at (lists, list length, k) = (2, 64, 64), (8, 64, 64), (8, 1024, 1024), P = 1 and
            16: after a warm-up, windows of back-to-back launches between two device events, time per launch, median
            (min - max) over the windows.
  query     ``identify(shortlist=64)`` of one probe over G entries of n keypoints (bf16 net, layout "f32"): the one
            index, then the same gallery as 2 and 4 shards on the one GPU (``ShardedGallery.split``, contiguous ranges),
            host clock around the call and a device synchronise, median (min - max).  A fresh process per round.
  unchanged with ``--parent TREE`` (a built checkout of the parent commit) the one-index call in that tree too, the two
            trees alternating; every process's runs are listed.  By the rule of DESIGN 5 a slowdown counts where the
            parent's median beats the new tree's best run by more than the new tree's own max - min.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "SHARDED_GALLERY_BENCH "


def _fmt(samples, unit="us"):
    scale = 1e6 if unit == "us" else 1e3
    return "%.1f (%.1f - %.1f) %s" % (statistics.median(samples) * scale, min(samples) * scale, max(samples) * scale, unit)


def _windows(torch, fn, launches=200, windows=21):
    """Seconds per launch of ``fn``: ``windows`` windows of ``launches`` back-to-back launches between device events."""
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / launches)
    return out


def _calls(torch, fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def child_query(args):
    """One process: the one-index call (and, on this tree, the same gallery as 2 and 4 shards) -> a JSON line."""
    sys.path.insert(0, args.tree)
    import torch
    import bench
    import fpm
    from fpm import params, synth
    dev = torch.device("cuda", 0)
    base = bench.make_gallery(args.seed, 1, args.distinct, args.n, 16)
    gallery = [base[i % len(base)] for i in range(args.gallery)]
    net = fpm.Net(regression=True, backbone=False, dtype="bf16")
    net.load_state_dict(params.init_params(args.seed))
    index = net.enroll(gallery, dev)
    probe = synth.make_graph(args.seed, 0, 0, args.n)
    torch.cuda.synchronize()

    def fresh(ix):
        for part in getattr(ix, "shards", [ix]):
            part._sel = None               # every timed query stages its entries, as a new probe's would
        return net.identify(probe, ix, topk=10, shortlist=64)
    res = dict(tree=args.child, one=_calls(torch, lambda: fresh(index), args.reps))
    if args.child == "new":
        for S in (2, 4):
            sg = fpm.ShardedGallery.split(index, [0] * S, "range")
            res["shards%d" % S] = _calls(torch, lambda: fresh(sg), args.reps)
            ref, got = fresh(index), fresh(sg)
            res["equal%d" % S] = all(torch.equal(got[k], ref[k]) for k in ("top_idx", "top_score", "short_idx", "cls_prob"))
            del sg
        res["one_again"] = _calls(torch, lambda: fresh(index), args.reps)
    print(TAG + json.dumps(res), flush=True)


def _spawn(args, which, tree, gallery):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--tree", tree, "--reps", str(args.reps),
           "--gallery", str(gallery), "--n", str(args.n), "--distinct", str(args.distinct), "--seed", str(args.seed)]
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    print("%s tree, %d entries: process done in %.0f s" % (which, gallery, time.perf_counter() - t0), file=sys.stderr,
          flush=True)
    for line in r.stdout.splitlines():
        if line.startswith(TAG):
            return json.loads(line[len(TAG):])
    raise RuntimeError("child %s failed (status %d):\n%s\n%s" % (which, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))


def kernel(lines):
    sys.path.insert(0, REPO)
    import ctypes
    import torch
    from fpm import _lib, ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(1)
    lib = _lib.load()
    V = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lines.append("topk_merge alone (device events, 21 windows of back-to-back launches, time per launch; 'C ABI': the entry "
                 "point on preallocated outputs, 'wrapper': the ops call with its checks and allocations)")
    for S, n, k in ((2, 64, 64), (8, 64, 64), (8, 1024, 1024)):
        for P in (1, 16):
            L = S * n
            # each list descending, the ids a random deal of 0 .. 4L over the lists, ascending inside a list's ties
            sc = torch.randn(P, S, n, generator=gen).sort(dim=2, descending=True).values.reshape(P, L).contiguous().to(dev)
            ids = torch.stack([torch.randperm(4 * L, generator=gen)[:L] for _ in range(P)]).to(torch.int32).to(dev)
            off = [t * n for t in range(S + 1)]
            offs = (ctypes.c_int * (S + 1))(*off)
            ti, ts, tc = (torch.empty(P, k, device=dev, dtype=torch.int32), torch.empty(P, k, device=dev),
                          torch.empty(P, k, device=dev, dtype=torch.int32))
            a = [V(sc), V(ids), L, P, offs, S, k, V(ti), V(ts), V(tc), st]
            t = _windows(torch, lambda: lib.fpm_topk_merge(*a))
            lines.append("  lists=%-2d length=%-4d k=%-4d P=%-2d  (%6.1f KB of keys in LDS)  C ABI   %s"
                         % (S, n, k, P, L * 8 / 1024.0, _fmt(t)))
            t = _windows(torch, lambda: ops.topk_merge(sc, ids, off, k), launches=100)
            lines.append("  lists=%-2d length=%-4d k=%-4d P=%-2d                              wrapper %s" % (S, n, k, P, _fmt(t)))


def _runs(samples):
    return " ".join("%.2f" % (v * 1e3) for v in samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r11_sharded_gallery.txt"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: the one-index call is timed there too")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--galleries", default="1024,16384")
    ap.add_argument("--gallery", type=int, default=1024)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--distinct", type=int, default=64, help="distinct graphs; the gallery repeats them")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--child", default=None, choices=["new", "parent"])
    ap.add_argument("--tree", default=REPO)
    args = ap.parse_args()
    if args.child:
        return child_query(args)
    lines = ["gallery over several GPUs: tools/sharded_gallery_bench.py on one MI355X; all times wall or device times of this "
             "run alone.  The shards share the one GPU: the sharded figures measure overhead only, no gain is expected or "
             "claimed; distinct devices are unmeasured (no multi-GPU box).", ""]
    # the query processes first: this process has not touched the GPU yet when it starts them
    for G in [int(g) for g in args.galleries.split(",")]:
        lines += ["query: identify(shortlist=64, topk=10), one probe x %d entries (%d distinct graphs), n = %d, bf16 net, layout "
                  "'f32'; host clock + synchronise, %d calls per process, median (min - max) ms; a fresh process per round"
                  % (G, args.distinct, args.n, args.reps)]
        new_runs, parent_runs = [], []
        for rnd in range(args.rounds):
            if args.parent:
                r = _spawn(args, "parent", os.path.abspath(args.parent), G)
                lines.append("  round %d  parent commit, one index (unchanged call)  %s" % (rnd, _fmt(r["one"], "ms")))
                lines.append("           runs: %s" % _runs(r["one"]))
                parent_runs.append(r["one"])
            r = _spawn(args, "new", REPO, G)
            lines.append("  round %d  this tree,     one index (unchanged call)  %s" % (rnd, _fmt(r["one"], "ms")))
            lines.append("           runs: %s" % _runs(r["one"]))
            for S in (2, 4):
                lines.append("  round %d  this tree,     %d shards on the one GPU     %s   (top_idx, top_score, short_idx, cls_prob "
                             "equal the one index's: %s)" % (rnd, S, _fmt(r["shards%d" % S], "ms"), r["equal%d" % S]))
            lines.append("  round %d  this tree,     one index again             %s" % (rnd, _fmt(r["one_again"], "ms")))
            new_runs.append(r["one"])
        if args.parent:
            new_all, par_all = sum(new_runs, []), sum(parent_runs, [])
            spread = max(new_all) - min(new_all)
            slow = statistics.median(par_all) < min(new_all) - spread
            lines.append("  unchanged call, all rounds: parent median %.2f ms; this tree median %.2f, best %.2f, max - min %.2f ms; "
                         "slowdown by the rule of DESIGN 5 (parent median < this tree's best - its max - min): %s"
                         % (statistics.median(par_all) * 1e3, statistics.median(new_all) * 1e3, min(new_all) * 1e3,
                            spread * 1e3, "YES" if slow else "no"))
        lines.append("")
    kernel(lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

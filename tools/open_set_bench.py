"""Open-set 1:N search: what the two kernels and the query layer's open-set stage cost, and what the z-score
says on the planted gallery.  Not part of ``bench.py``; nothing here is asserted anywhere.

    python tools/open_set_bench.py [--out FILE] [--parent TREE] [--rounds N]

Writes a text report (default ``profiles/r10_open_set.txt``):

  kernels   ``ops.cohort_decide`` at P = 1 and 1024, K = 96 (k = 10, skip 1, cohort 32, with a threshold) and
            ``ops.group_topr`` at P = 16, S = 4096, c = 4, r = 2, each alone on the device: after a warm-up, windows
            of back-to-back launches between two device events, time per launch, median (min - max) over the windows.
  query     ``identify(by="subject", fuse="mean", shortlist=64)`` of one probe over 1024 entries of n keypoints, four
            impressions per subject, host clock around the call and a device synchronise, median (min - max): the
            unchanged call, then the call with ``top_r=2, normalize="cohort", threshold=3.0``; their difference is the
            cost of the added stage per query.  Each in a fresh process per round (``--rounds``), and with ``--parent
            TREE`` (a built checkout of the parent commit) the unchanged call in that tree, alternating with this one.
  planted   on the planted gallery of ``tests/test_shortlist_gpu.planted()`` (40 entries, labels ``entry // 3``, the
            three probes' mates at entries 7, 19 and 38): each probe's rank-1 subject and its z with the mate's
            subject selected and deselected (``shortlist=8, top_r=2, cohort=6``), f32 net, the tests' "spread" weights.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _query_setup(tree, args):
    sys.path.insert(0, tree)
    import torch
    import bench
    import fpm
    from fpm import params, synth
    dev = torch.device("cuda", 0)
    base = bench.make_gallery(args.seed, 1, args.distinct, args.n, 16)
    gallery = [base[i % len(base)] for i in range(args.gallery)]
    net = fpm.Net(regression=True, backbone=False, dtype="bf16")
    net.load_state_dict(params.init_params(args.seed))
    index = net.enroll(gallery, dev, subjects=[i // 4 for i in range(args.gallery)])
    probe = synth.make_graph(args.seed, 0, 0, args.n)
    torch.cuda.synchronize()
    return torch, net, index, probe


def child_query(args):
    """One process: the unchanged call (and, on this tree, the call with the open-set arguments) -> a JSON line."""
    torch, net, index, probe = _query_setup(args.tree, args)
    kw = dict(topk=10, shortlist=64, by="subject", fuse="mean")

    def fresh(**more):
        index._sel = None                  # every timed query stages its entries, as a new probe's would
        return net.identify(probe, index, **kw, **more)
    res = dict(tree=args.child, plain=_calls(torch, fresh, args.reps))
    if args.child == "new":
        res["open"] = _calls(torch, lambda: fresh(top_r=2, normalize="cohort", threshold=3.0), args.reps)
        res["plain_again"] = _calls(torch, fresh, args.reps)
    print("OPEN_SET_BENCH " + json.dumps(res), flush=True)


def _spawn(args, which, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--tree", tree, "--reps", str(args.reps),
           "--gallery", str(args.gallery), "--n", str(args.n), "--distinct", str(args.distinct), "--seed", str(args.seed)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    for line in r.stdout.splitlines():
        if line.startswith("OPEN_SET_BENCH "):
            return json.loads(line[len("OPEN_SET_BENCH "):])
    raise RuntimeError("child %s failed (status %d):\n%s\n%s" % (which, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))


def kernels(lines):
    sys.path.insert(0, REPO)
    import ctypes
    import torch
    from fpm import _lib, ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(1)
    lib = _lib.load()
    V = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lines.append("kernels alone (device events, 21 windows of back-to-back launches, time per launch; 'C ABI': the entry point "
                 "on preallocated outputs, 'wrapper': the ops call with its checks and allocations)")
    for P in (1, 1024):
        top = torch.randn(P, 96, generator=gen).sort(dim=1, descending=True).values.contiguous().to(dev)
        z, acc = torch.empty(P, 10, device=dev), torch.empty(P, 10, device=dev, dtype=torch.int32)
        mu, sg, cn = torch.empty(P, device=dev), torch.empty(P, device=dev), torch.empty(P, device=dev, dtype=torch.int32)
        a = [V(top), P, 96, 10, 1, 32, 1e-6, 1, 1, 3.0, V(z), V(mu), V(sg), V(cn), V(acc), st]
        t = _windows(torch, lambda: lib.fpm_cohort_decide(*a))
        lines.append("  cohort_decide P=%-4d K=96 k=10 skip=1 cohort=32 threshold   C ABI   %s" % (P, _fmt(t)))
        t = _windows(torch, lambda: ops.cohort_decide(top, 10, 1, 32, 1e-6, 3.0))
        lines.append("  cohort_decide P=%-4d K=96 k=10 skip=1 cohort=32 threshold   wrapper %s" % (P, _fmt(t)))
    P, S, c = 16, 4096, 4
    s = torch.randn(P, S * c, generator=gen).to(dev)
    off = (torch.arange(S + 1, dtype=torch.int32) * c)
    pos = torch.arange(S * c, dtype=torch.int32)
    off_d, pos_d = off.to(dev), pos.to(dev)
    gs, gb = torch.empty(P, S, device=dev), torch.empty(P, S, device=dev, dtype=torch.int32)
    for name, r in (("group_topr r=2", 2), ("group_topr r=16", 16)):
        a = [V(s), S * c, P, S * c, V(off_d), 0, V(pos_d), 0, S, r, V(gs), V(gb), st]
        t = _windows(torch, lambda: lib.fpm_group_topr(*a))
        lines.append("  %-30s P=16 S=4096 c=4   C ABI   %s" % (name, _fmt(t)))
    a = [V(s), S * c, P, S * c, V(off_d), 0, V(pos_d), 0, S, 1, V(gs), V(gb), st]
    t = _windows(torch, lambda: lib.fpm_group_scores(*a))
    lines.append("  %-30s P=16 S=4096 c=4   C ABI   %s" % ("group_scores mean (for scale)", _fmt(t)))
    for name, fn in (("group_topr r=2", lambda: ops.group_topr(s, off_d, pos_d, 2, gscore=gs, gbest=gb, off_host=off, pos_host=pos)),
                     ("group_scores mean (for scale)", lambda: ops.group_scores(s, off_d, pos_d, "mean", gscore=gs, gbest=gb,
                                                                                off_host=off, pos_host=pos))):
        t = _windows(torch, fn, launches=50)
        lines.append("  %-30s P=16 S=4096 c=4   wrapper %s   (the host check of the tables)" % (name, _fmt(t)))


def planted(lines):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    from test_shortlist_cpu import state_dicts
    from test_shortlist_gpu import MATES, _net, planted as make
    dev = torch.device("cuda", 0)
    gal, probes = make()
    net = _net(state_dicts()["spread"], "f32")
    labels = [e // 3 for e in range(len(gal))]
    index = net.enroll(gal, dev, batch=16, subjects=labels)
    kw = dict(topk=5, shortlist=8, by="subject", fuse="mean", top_r=2, normalize="cohort", cohort=6, cohort_skip=1)
    lines.append("planted gallery (40 entries, labels entry // 3; identify(%s)); random weights: the exact scores are "
                 "nearly flat and carry no meaning, so neither does the z (only the coarse stage finds the mates)"
                 % ", ".join("%s=%r" % kv for kv in kw.items()))
    for e, p in sorted(MATES.items(), key=lambda kv: kv[1]):
        mate = labels[e]
        for what, sel in (("selected  ", None), ("deselected", [i for i in range(len(gal)) if labels[i] != mate])):
            r = net.identify(probes[p], index, select=sel, **kw)
            lines.append("  probe %d, mate's subject %2d %s: rank-1 subject %2d, score %.4f, z %8.3f, cohort mu %.6f sigma %.3g n %d"
                         % (p, mate, what, int(r["top_subject"][0]), float(r["top_score"][0]), float(r["top_z"][0]),
                            float(r["cohort_mu"]), float(r["cohort_sigma"]), int(r["cohort_n"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r10_open_set.txt"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: the unchanged call is timed there too")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--gallery", type=int, default=1024)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--distinct", type=int, default=64, help="distinct graphs; the gallery repeats them")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--child", default=None, choices=["new", "parent"])
    ap.add_argument("--tree", default=REPO)
    args = ap.parse_args()
    if args.child:
        return child_query(args)
    lines = ["open-set search: tools/open_set_bench.py on one MI355X; all times wall or device times of this run alone",
             ""]
    # the query processes first: this process has not touched the GPU yet when it starts them
    lines += ["query: identify(by='subject', fuse='mean', shortlist=64), one probe x %d entries (%d distinct graphs), n = %d, "
              "four impressions per subject, bf16 net; host clock + synchronise, %d calls per process, median (min - max)"
              % (args.gallery, args.distinct, args.n, args.reps)]
    plain, opened = [], []
    for rnd in range(args.rounds):
        if args.parent:
            r = _spawn(args, "parent", os.path.abspath(args.parent))
            lines.append("  round %d  parent commit, unchanged call            %s" % (rnd, _fmt(r["plain"], "ms")))
        r = _spawn(args, "new", REPO)
        lines.append("  round %d  this tree,     unchanged call            %s" % (rnd, _fmt(r["plain"], "ms")))
        lines.append("  round %d  this tree,     top_r + cohort + threshold %s" % (rnd, _fmt(r["open"], "ms")))
        lines.append("  round %d  this tree,     unchanged call again      %s" % (rnd, _fmt(r["plain_again"], "ms")))
        plain += r["plain"] + r["plain_again"]
        opened += r["open"]
    lines.append("  added stage (median with - median without, this tree, all rounds): %.0f us per query"
                 % ((statistics.median(opened) - statistics.median(plain)) * 1e6))
    lines.append("")
    kernels(lines)
    lines.append("")
    planted(lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

"""1:N identification: the cached-gallery forward (``Net.identify`` over an enrolled
``GalleryIndex``) against the uncached probe x gallery forward (``Net.run`` over
``DeviceBatch.from_probe_gallery``) on the same graphs.  GPU.

    python tools/identify_bench.py [--gallery 1024] [--n 128] [--reps 7] [--out profiles/identify_c4.json]
    python tools/identify_bench.py --shortlist 64 [--large 16384]      (-> profiles/identify_shortlist.json)
    python tools/identify_bench.py --shortlist 64 --coarse wide --n 256 --large 4096
                                                                       (-> profiles/identify_shortlist_wide.json)
    python tools/identify_bench.py --shortlist 64 --coarse stream --n 512 --large 4096
    python tools/identify_bench.py --shortlist 64 --coarse stream --n 256 --large 0 --append
                                                                       (-> profiles/identify_shortlist_stream.json)
    python tools/identify_bench.py --shortlist 64 --layout f32,f32+bf16,bf16+host [--coarse auto --n 256] [--append]
                                                                       (-> profiles/identify_compact.json)
    python tools/identify_bench.py --shortlist 64 --layout bf16+host,fp8+host [--coarse stream --n 512] [--append]
                                                                       (-> profiles/identify_fp8.json)
    python tools/identify_bench.py --probes 16 --shortlist 64 [--coarse auto --n 256 --large 0] [--append]
                                                                       (-> profiles/identify_many.json)
    python tools/identify_bench.py --subjects 4 --shortlist 64 --probes 16 --gallery 16384 --large 0 --dtypes bf16
                                                                       (-> profiles/identify_subjects.json)
    python tools/identify_bench.py --shortlist 64 --prescreen 1024 --layout fp8+host --dtypes bf16
    python tools/identify_bench.py --shortlist 64 --prescreen 1024 --layout fp8+host --dtypes bf16 --coarse stream
                                   --n 512 --large 4096 --append       (-> profiles/identify_prescreen.json)

``--prescreen K`` (with ``--shortlist M``; one ``--layout``, the ``--large`` gallery alone): the index enrolled with
descriptors; ``identify(shortlist=M, prescreen=K)`` against ``identify(shortlist=M)`` (the path without the
prescreen: its kernels are untouched) in one process, with the A/B verdict; the prescreen's three kernels each alone
and together as the query runs them, the coarse pass over the K kept entries against the pass over the whole
gallery, and ``add_descriptors`` once.  Also the descriptor scores of mate and runner-up on the tests' planted-mate
gallery.  Recall on trained weights is not measured: the weights are ``params.init_params``.

``--subjects R`` (with ``--shortlist M``): the gallery labelled with R consecutive entries per subject.
``ops.group_scores`` (max and mean) and ``ops.rank_select`` timed on the same ``--probes`` x gallery coarse
matrix, and one probe's subject-level shortlisted query (``impressions`` all and best) against the
entry-level one at the same M.

``--probes Q`` (with ``--shortlist M``): a probe set.  The looped ``identify(list of Q probes, shortlist=M)``
(one probe at a time: the path before probe sets) against ``identify_many`` over the same enrolled gallery
in one process; per probe the whole query, the coarse pass (``coarse_scores`` looped against
``coarse_scores_many``) and the exact stage (Q forwards of M pairs against the grouped forwards of
``identify_many``'s own pair lists), with the A/B verdict of each; and once the coarse pass with the pairs
of a launch in entry-major order (an entry's probes on one XCD) against the default probe-major order.

``--shortlist M``: by the same protocol, the shortlisted query ``identify(shortlist=M)`` against the
full ``identify`` in one process, at the C4 shape and at a larger gallery, with the coarse pass
(ms and index bytes per second), the selection and the M-pair forward each timed alone.
``--coarse wide|auto`` runs the coarse pass on ``fpm_coarse_score_wide`` (boxes of up to 256 keypoints)
and adds that kernel alone on synthetic rows; at n <= 128 it also times the fused coarse pass over the
same gallery, the number that decides which kernel small boxes take.
``--coarse stream|any`` runs it on ``fpm_coarse_score_stream`` (boxes of up to 600 keypoints; the full
``identify`` is then the only other query there is) and adds that kernel alone on synthetic rows; at
n <= 256 it also times the wide coarse pass and the wide kernel alone over the same gallery, stream
against wide in one process: the number that decides which kernel boxes of up to 256 take.

``--layout a,b,..`` (with ``--shortlist``): the index layouts against each other.  The gallery is enrolled
once per layout in one process; per layout the device and host bytes held, the coarse pass (which reads
the bf16 rows where the layout has them), the fetch of the shortlist's fp32 rows from pinned host memory
("bf16+host", "fp8+host"), the M-pair forward and the whole shortlisted query; an "fp8+host" layout also records
how far its coarse scores lie from the baseline's and how much of the coarse top 10 they share, on this gallery
and on the tests' planted-mate gallery; the first layout is the baseline of
the A/B verdicts.

Shape: config C4 (one probe, n = 128 keypoints, a gallery of 1024), both dtypes.  Per dtype, in a
fresh child process under its own time limit: one warm-up, then ``--reps`` (>= 5) timed forwards of
each path, HIP events around each forward (the forward ends with its host Hungarian, so the events
bracket the whole forward); medians and the spread are reported.  ``identify`` is timed as a query
is served -- it stages the probe, gathers, runs the forward and ranks; the uncached ``run`` is timed
on a batch staged beforehand (``from_probe_gallery``'s staging is not timed).  Then, outside the timed
runs: the per-stage marks of a one-chunk, one-stream forward of both paths (``Net._mark`` events) and
the gather kernel alone (achieved GB/s).  The parent writes one JSON file; a failing child ends the
run (nothing else is started on the GPU after it).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _timed(fn, reps):
    """[(GPU ms between events around fn, wall ms)] of ``reps`` calls."""
    import time
    import torch
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append((e0.elapsed_time(e1), (time.perf_counter() - t) * 1e3))
    return out


def _summary(samples, pairs):
    ev = sorted(s[0] for s in samples)
    med = statistics.median(ev)
    return dict(event_ms=[round(x, 3) for x in ev], median_ms=round(med, 3), min_ms=round(ev[0], 3),
                max_ms=round(ev[-1], 3), wall_median_ms=round(statistics.median(s[1] for s in samples), 3),
                pairs_per_s=round(pairs / med * 1e3, 1))


def _marks(net, fn, reps=3):
    """Mean GPU ms between consecutive stage marks of a one-chunk, one-stream forward."""
    import collections
    keep = (net._stage_events, net.tail_streams, net.tail_groups)
    net._stage_events, net.tail_streams, net.tail_groups = True, 1, 1
    try:
        fn()
        net.stage_events()
        acc = collections.OrderedDict()
        for _ in range(reps):
            fn()
            for name, ms in net.stage_events():
                acc[name] = acc.get(name, 0.0) + ms / reps
    finally:
        net._stage_events, net.tail_streams, net.tail_groups = keep
        net._ev_marks = []
    return {k: round(v, 3) for k, v in acc.items()}


def child(args):
    import time
    import torch
    import bench
    import fpm
    from fpm import ops, params, synth
    from fpm.batch import DeviceBatch
    dev = torch.device("cuda", 0)
    G, n, dtype = args.gallery, args.n, args.child
    probe = synth.make_graph(args.seed, 0, 0, n)
    gallery = bench.make_gallery(args.seed, 1, G, n, args.gen_workers)
    net = fpm.Net(regression=True, backbone=False, dtype=dtype)
    net.load_state_dict(params.init_params(args.seed))
    t = time.perf_counter()
    index = net.enroll(gallery, dev)
    torch.cuda.synchronize()
    enroll_s = time.perf_counter() - t
    bt = DeviceBatch.from_probe_gallery(probe, gallery, dev)
    del gallery
    res = dict(dtype=dtype, gallery=G, n=n, sc_mode=index.sc_mode, reps=args.reps, enroll_s=round(enroll_s, 3),
               index_mb=round(index.nbytes() / 2 ** 20, 1), chunks=net.pipeline_chunks(G))
    ref = net.run(bt)                                   # the warm-up of each path, compared
    out = net.identify(probe, index, topk=10)
    torch.cuda.synchronize()
    res["identical"] = all(bool(torch.equal(out[k], ref[k])) for k in ("ss", "ds_mat", "perm_mat", "k_prob", "cls_prob"))
    res["top_idx"] = out["top_idx"].tolist()
    del ref, out
    unc = _timed(lambda: net.run(bt), args.reps)
    cac = _timed(lambda: net.identify(probe, index, topk=10), args.reps)
    res["uncached"], res["cached"] = _summary(unc, G), _summary(cac, G)
    res["speedup_median"] = round(res["uncached"]["median_ms"] / res["cached"]["median_ms"], 3)
    # faster by more than the spread: the slowest cached forward beats the fastest uncached one
    res["cached_faster_beyond_spread"] = res["cached"]["max_ms"] < res["uncached"]["min_ms"]
    res["marks_uncached_ms"] = _marks(net, lambda: net.run(bt, chunks=1))
    res["marks_cached_ms"] = _marks(net, lambda: net.identify(probe, index, topk=10, chunks=1))
    # the gather kernel alone, in the shape of side 1 of this forward
    split = net._kp_split(1, bt)
    opdt = torch.float32 if index.sc_mode == "f32" else torch.bfloat16
    cols = 2304 if split else 768
    out_t = torch.empty(G * n, cols, device=dev, dtype=opdt)
    idx = torch.arange(G, dtype=torch.int32, device=dev)
    call = lambda: ops.rows_gather_scale(index.y, index.row_off, idx, n, out_t=out_t, split=split,
                                         idx_host=idx.cpu(), row_off_host=index.row_off_host)
    call()
    ks = sorted(s[0] for s in _timed(call, 20))
    nbytes = index.y.numel() * 4 + out_t.numel() * out_t.element_size()
    res["gather"] = dict(split=split, out_dtype=str(opdt).replace("torch.", ""), bytes=nbytes,
                         median_ms=round(statistics.median(ks), 4), min_ms=round(ks[0], 4),
                         gb_per_s=round(nbytes / statistics.median(ks) / 1e6, 1),
                         note="events around one launch: launch latency included")
    print("IDENTIFY_BENCH " + json.dumps(res), flush=True)


def _ev(samples):
    ev = sorted(s[0] for s in samples)
    return dict(event_ms=[round(x, 3) for x in ev], in_order_ms=[round(s[0], 3) for s in samples],
                median_ms=round(statistics.median(ev), 3), min_ms=round(ev[0], 3), max_ms=round(ev[-1], 3),
                wall_median_ms=round(statistics.median(s[1] for s in samples), 3))


def child_shortlist(args):
    """``--shortlist M``: the shortlisted query (coarse pass, selection, M-pair forward) against the
    full ``identify`` over the same gallery, in this one process; and each part alone."""
    import torch
    import bench
    import fpm
    from fpm import ops, params, synth
    dev = torch.device("cuda", 0)
    G, n, dtype, M, coarse = args.gallery, args.n, args.child, args.shortlist, args.coarse
    probe = synth.make_graph(args.seed, 0, 0, n)
    base = bench.make_gallery(args.seed, 1, min(G, args.distinct), n, args.gen_workers)
    gallery = [base[i % len(base)] for i in range(G)]      # past --distinct graphs the gallery repeats them
    net = fpm.Net(regression=True, backbone=False, dtype=dtype)
    net.load_state_dict(params.init_params(args.seed))
    index = net.enroll(gallery, dev)
    torch.cuda.synchronize()
    del gallery, base
    row_bytes = int(index.y.numel()) * 4
    res = dict(dtype=dtype, gallery=G, distinct_graphs=min(G, args.distinct), n=n, shortlist=M, sc_mode=index.sc_mode,
               reps=args.reps, index_mb=round(index.nbytes() / 2 ** 20, 1), row_bytes=row_bytes, coarse=coarse)
    # warm-ups; the full query last, so its timed runs find the index's whole-gallery selection staged
    # (as a service that only runs full queries would), not the shortlist's
    short = net.identify(probe, index, topk=10, shortlist=M, coarse=coarse)
    full = net.identify(probe, index, topk=10)
    torch.cuda.synchronize()
    sidx = short["short_idx"]
    res["full_top10"] = full["top_idx"].tolist()
    res["short_top10"] = short["top_idx"].tolist()
    res["full_top10_in_shortlist"] = len(set(full["top_idx"].tolist()) & set(sidx.tolist()))
    call = short["coarse_all"].view(1, -1).clone()
    del full, short

    def series(fn):
        # one warm-up of this very call, then the timed queries
        fn()
        torch.cuda.synchronize()
        return _ev(_timed(fn, args.reps))

    def fresh(fn):
        # a repeated probe repeats its shortlist; drop the index's staged selection so that every
        # timed shortlisted query stages its M entries, as a new probe's would
        index._sel = None
        return fn()
    # the full query keeps the index's whole-gallery selection staged across its runs, as a service
    # that only runs full queries would
    res["full"] = series(lambda: net.identify(probe, index, topk=10))
    res["shortlisted"] = series(lambda: fresh(lambda: net.identify(probe, index, topk=10, shortlist=M,
                                                                   coarse=coarse)))

    def coarse_pass(route):
        r = series(lambda: net.coarse_scores(probe, index, coarse=route))
        r["index_tb_per_s"] = round(row_bytes / r["median_ms"] / 1e9, 3)
        r["fraction_of_5p5_tb_per_s"] = round(r["index_tb_per_s"] / 5.5, 3)
        return r
    res["coarse"] = coarse_pass(coarse)

    def kernel_alone(op):
        # one coarse kernel alone: synthetic rows (N(0, 0.05)), min(G, 1024) entries of n keypoints, one launch
        Gs = min(G, 1024)
        ys = torch.randn(Gs * n, 768, device=dev) * 0.05
        offs = torch.arange(Gs + 1, dtype=torch.int64) * n
        ids = torch.arange(Gs, dtype=torch.int32)
        offs_d, ids_d = offs.to(dev), ids.to(dev)
        yps = torch.randn(n, 768, device=dev) * 0.05
        cfs = torch.tanh(torch.randn(Gs, 768, device=dev))
        outs = torch.empty(Gs, device=dev)
        r = series(lambda: op(ys, offs_d, ids_d, yps, cfs, tau=net.tau, out=outs, idx_host=ids, row_off_host=offs))
        kb = int(ys.numel()) * 4
        r.update(entries=Gs, row_bytes=kb, rows_tb_per_s=round(kb / r["median_ms"] / 1e9, 3),
                 us_per_pair_per_cu=round(r["median_ms"] * 1e3 * 256 / Gs, 1),
                 note="events around one launch: launch latency and the scratch allocation included")
        return r
    if coarse in ("wide", "auto"):
        if n <= ops.COARSE_NMAX:
            # the same gallery through the fused kernel: which of the two small boxes should take
            res["coarse_fused"] = coarse_pass("fused")
            res["wide_over_fused"] = round(res["coarse"]["median_ms"] / res["coarse_fused"]["median_ms"], 3)
        res["wide_kernel"] = kernel_alone(ops.coarse_score_wide)
    if coarse in ("stream", "any"):
        res["stream_kernel"] = kernel_alone(ops.coarse_score_stream)
        if n <= ops.COARSE_WIDE_NMAX:
            # the same gallery through the wide kernel: which of the two boxes of up to 256 should take
            res["coarse_stream"] = res["coarse"] if coarse == "stream" else coarse_pass("stream")
            res["coarse_wide"] = coarse_pass("wide")
            res["stream_over_wide"] = round(res["coarse_stream"]["median_ms"] / res["coarse_wide"]["median_ms"], 3)
            res["wide_kernel"] = kernel_alone(ops.coarse_score_wide)
            res["stream_kernel_over_wide_kernel"] = round(res["stream_kernel"]["median_ms"]
                                                          / res["wide_kernel"]["median_ms"], 3)
    res["select"] = series(lambda: ops.rank_select(call, M))
    res["forward_M"] = series(lambda: fresh(lambda: net.identify(probe, index, topk=10, select=sidx)))
    f, s = res["full"], res["shortlisted"]
    res["speedup_median"] = round(f["median_ms"] / s["median_ms"], 2)
    # the project's A/B rule: the candidate's median beats the baseline's best run by more than the
    # baseline's own spread
    res["ab_margin_ms"] = round(f["min_ms"] - (f["max_ms"] - f["min_ms"]) - s["median_ms"], 3)
    res["ab_pass"] = res["ab_margin_ms"] > 0
    print("IDENTIFY_BENCH " + json.dumps(res), flush=True)


def child_layouts(args):
    """``--shortlist M --layout a,b,..``: the same gallery enrolled once per index layout in this one
    process; per layout the device / host bytes held, the coarse pass, the fetch of the M shortlisted
    entries' rows (layouts with the fp32 rows on the host), the M-pair forward and the whole
    shortlisted query.  The first layout listed is the baseline of the A/B margins (the project's
    rule: the candidate's median against the baseline's best run less the baseline's spread)."""
    import torch
    import bench
    import fpm
    from fpm import gallery as fgallery, params, synth
    dev = torch.device("cuda", 0)
    G, n, dtype, M, coarse = args.gallery, args.n, args.child, args.shortlist, args.coarse
    layouts = args.layout.split(",")
    probe = synth.make_graph(args.seed, 0, 0, n)
    base = bench.make_gallery(args.seed, 1, min(G, args.distinct), n, args.gen_workers)
    gallery = [base[i % len(base)] for i in range(G)]      # past --distinct graphs the gallery repeats them
    net = fpm.Net(regression=True, backbone=False, dtype=dtype)
    net.load_state_dict(params.init_params(args.seed))
    res = dict(dtype=dtype, gallery=G, distinct_graphs=min(G, args.distinct), n=n, shortlist=M, reps=args.reps,
               coarse=coarse, layouts={})
    index = {}
    for lay in layouts:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        index[lay] = net.enroll(gallery, dev, layout=lay)
        torch.cuda.synchronize()
        ix = index[lay]
        res["layouts"][lay] = dict(nbytes=ix.nbytes(), host_nbytes=ix.host_nbytes(),
                                   enroll_peak_device_bytes=torch.cuda.max_memory_allocated(dev) - before,
                                   templates_per_288_gb=int(288e9 / (ix.nbytes() / G)))
    del gallery, base
    res["sc_mode"] = index[layouts[0]].sc_mode
    res["row_bytes"] = int(index[layouts[0]].y.numel()) * 4

    def series(fn):
        fn()
        torch.cuda.synchronize()
        return _ev(_timed(fn, args.reps))

    def fresh(ix, fn):
        # a new probe's shortlist: neither the selection's batch nor its staged rows are kept
        ix._sel = ix._stage = None
        return fn()
    ref = None
    for lay in layouts:
        ix, r = index[lay], res["layouts"][lay]
        short = net.identify(probe, ix, topk=10, shortlist=M, coarse=coarse)
        torch.cuda.synchronize()
        sidx = short["short_idx"].cpu().long()
        ref = short if ref is None else ref
        r["identical_to_%s" % layouts[0]] = all(bool(torch.equal(short[k], ref[k])) for k in
                                                ("ss", "ds_mat", "perm_mat", "k_prob", "cls_prob", "top_idx",
                                                 "top_score", "short_idx", "coarse_score", "coarse_all"))
        if lay == fgallery.FP8_LAYOUT and ref is not short:
            # the coarse scores are another operand's; the exact outputs of an entry are the same bits
            r["coarse_vs_%s" % layouts[0]] = _coarse_shift(short["coarse_all"], ref["coarse_all"])
            sel = net.identify(probe, index[layouts[0]], topk=10, select=sidx)
            r["exact_identical_on_own_shortlist"] = all(bool(torch.equal(short[k], sel[k])) for k in
                                                        ("ss", "ds_mat", "perm_mat", "k_prob", "cls_prob", "top_idx",
                                                         "top_score"))
        r["coarse"] = series(lambda: net.coarse_scores(probe, ix, coarse=coarse))
        read = res["row_bytes"] // (1 if ix.y16 is None else 2)
        if ix.y8 is not None:
            read = int(ix.y8.shape[0]) * fgallery.ROW_BYTES_FP8
        r["device_row_bytes_per_keypoint"] = {"f32": 3072, "f32+bf16": 4608, "bf16+host": 1536,
                                              "fp8+host": fgallery.ROW_BYTES_FP8}[lay]
        r["coarse"].update(index_bytes_read=read, index_tb_per_s=round(read / r["coarse"]["median_ms"] / 1e9, 3))
        if lay in fgallery.HOST_LAYOUTS:
            r["fetch"] = series(lambda: fresh(ix, lambda: ix.fetch(sidx)))
            fb = int(ix.n[sidx].sum()) * 3072
            r["fetch"].update(bytes=fb, gb_per_s=round(fb / r["fetch"]["median_ms"] / 1e6, 1),
                              note="pinned host rows read by the kernel; events around one fetch: the offsets' "
                                   "upload and the launch latency included")
        r["forward_M"] = series(lambda: fresh(ix, lambda: net.identify(probe, ix, topk=10, select=sidx)))
        r["shortlisted"] = series(lambda: fresh(ix, lambda: net.identify(probe, ix, topk=10, shortlist=M,
                                                                         coarse=coarse)))
        del short
    b = res["layouts"][layouts[0]]
    for lay in layouts[1:]:
        r = res["layouts"][lay]
        for part in ("coarse", "forward_M", "shortlisted"):
            o, c = b[part], r[part]
            r["ab_%s" % part] = dict(
                baseline=layouts[0], speedup_median=round(o["median_ms"] / c["median_ms"], 3),
                faster_margin_ms=round(o["min_ms"] - (o["max_ms"] - o["min_ms"]) - c["median_ms"], 3),
                slower_margin_ms=round(c["min_ms"] - (c["max_ms"] - c["min_ms"]) - o["median_ms"], 3))
            r["ab_%s" % part]["verdict"] = ("faster" if r["ab_%s" % part]["faster_margin_ms"] > 0 else
                                            "slower" if r["ab_%s" % part]["slower_margin_ms"] > 0 else "within spread")
    if fgallery.FP8_LAYOUT in layouts[1:]:
        res["planted"] = _planted_shift(layouts[0], dtype)
    print("IDENTIFY_BENCH " + json.dumps(res), flush=True)


def _coarse_shift(got, ref):
    """One probe's coarse scores on two layouts -> the largest shift and how much of the top 10 is shared."""
    import torch
    k = min(10, int(ref.numel()))
    a, b = set(torch.topk(got, k).indices.tolist()), set(torch.topk(ref, k).indices.tolist())
    return dict(max_shift=float((got - ref).abs().max()), ref_min=float(ref.min()), ref_max=float(ref.max()),
                top10_overlap=len(a & b))


def _planted_shift(base, dtype):
    """The tests' planted-mate gallery (40 entries, three probes, the "spread" weights) on the fp8 layout against
    ``base``: per probe the coarse-score shift, the top-10 overlap and the mate's margin."""
    import torch
    import fpm
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from test_shortlist_cpu import state_dicts
    from test_shortlist_gpu import MATES, planted
    dev = torch.device("cuda", 0)
    gal, probes = planted()
    net = fpm.Net(regression=True, backbone=False, dtype=dtype)
    net.load_state_dict(state_dicts()["spread"])
    a, b = net.enroll(gal, dev, batch=16, layout="fp8+host"), net.enroll(gal, dev, batch=16, layout=base)
    out = []
    for p, probe in enumerate(probes):
        got, ref = net.coarse_scores(probe, a)[0], net.coarse_scores(probe, b)[0]
        mate = [e for e, q in MATES.items() if q == p][0]
        rest = torch.cat([got[:mate], got[mate + 1:]])
        out.append(dict(_coarse_shift(got, ref), mate_first=int(torch.argmax(got)) == mate, mate_score=float(got[mate]),
                        best_other=float(rest.max())))
    return dict(gallery=len(gal), baseline=base, weights="spread", probes=out)


def _entry_major(p0, p1, Qs, Gs):
    """``gallery._coarse_pairs_order``'s alternative: blocks of 8 entries x Qs probes, place r of a
    block is (probe r // 8, entry r % 8), so that with one workgroup per pair and workgroups dealt to
    the 8 XCDs in turn an entry's probes run on one XCD (its rows in that XCD's L2)."""
    import torch
    lin = torch.arange(p0, p1, dtype=torch.int64)
    blk = torch.div(lin, 8 * Qs, rounding_mode="floor")
    ne = torch.clamp(Gs - 8 * blk, max=8)
    r = lin - blk * 8 * Qs
    qi, gi = torch.div(r, ne, rounding_mode="floor"), 8 * blk + r % ne
    return qi, gi, qi * Gs + gi


def child_probes(args):
    """``--probes Q --shortlist M``: looped identify against identify_many, in this one process."""
    import torch
    import bench
    import fpm
    from fpm import gallery as gal_mod
    from fpm import params, synth
    dev = torch.device("cuda", 0)
    G, n, dtype, M, coarse, Q = args.gallery, args.n, args.child, args.shortlist, args.coarse, args.probes
    probes = [synth.make_graph(args.seed, p, 0, n) for p in range(Q)]
    base = bench.make_gallery(args.seed, 1, min(G, args.distinct), n, args.gen_workers)
    gallery = [base[i % len(base)] for i in range(G)]      # past --distinct graphs the gallery repeats them
    net = fpm.Net(regression=True, backbone=False, dtype=dtype)
    net.load_state_dict(params.init_params(args.seed))
    index = net.enroll(gallery, dev)
    pset = net.enroll(probes, dev)
    torch.cuda.synchronize()
    del gallery, base
    res = dict(dtype=dtype, gallery=G, distinct_graphs=min(G, args.distinct), n=n, probes=Q, shortlist=M,
               sc_mode=index.sc_mode, reps=args.reps, coarse=coarse, group_pairs=args.group_pairs)
    loop = net.identify(probes, index, topk=10, shortlist=M, coarse=coarse)
    many = net.identify_many(pset, index, topk=10, shortlist=M, coarse=coarse, group_pairs=args.group_pairs)
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int32)
    res["same_shortlists"] = all(bool(torch.equal(a["short_idx"], b["short_idx"])) for a, b in zip(loop, many))
    res["same_coarse_bits"] = all(bool(torch.equal(bits(a["coarse_all"]), bits(b["coarse_all"])))
                                  for a, b in zip(loop, many))
    res["same_top10"] = sum(a["top_idx"].tolist() == b["top_idx"].tolist() for a, b in zip(loop, many))
    short = [a["short_idx"].cpu().long() for a in loop]
    groups = gal_mod.probe_groups(pset.n, M, args.group_pairs)
    res["groups"] = [len(g) for g in groups]
    lists = [torch.stack([torch.tensor(g).view(-1, 1).expand(-1, short[0].numel()).reshape(-1),
                          torch.cat([short[i] for i in g])], 1) for g in groups]
    del loop, many

    def series(fn):
        # one warm-up of this very call, then the timed runs; per probe
        fn()
        torch.cuda.synchronize()
        r = _ev(_timed(fn, args.reps))
        r["per_probe_ms"] = "%.3f (%.3f - %.3f)" % (r["median_ms"] / Q, r["min_ms"] / Q, r["max_ms"] / Q)
        return r

    def exact_loop():
        for p, s_ in zip(probes, short):
            net.identify(p, index, topk=10, select=s_)

    def exact_many():
        for pairs in lists:
            gal_mod._run_pairs(net, pset, index, pairs, None)
    parts = dict(
        query=(lambda: net.identify(probes, index, topk=10, shortlist=M, coarse=coarse),
               lambda: net.identify_many(pset, index, topk=10, shortlist=M, coarse=coarse,
                                         group_pairs=args.group_pairs)),
        coarse_pass=(lambda: net.coarse_scores(probes, index, coarse=coarse),
                     lambda: net.coarse_scores_many(pset, index, coarse=coarse)),
        exact_stage=(exact_loop, exact_many))

    def verdict(o, c):
        # the project's A/B rule: the candidate's median against the baseline's best run less its spread
        faster = o["min_ms"] - (o["max_ms"] - o["min_ms"]) - c["median_ms"]
        slower = c["min_ms"] - (c["max_ms"] - c["min_ms"]) - o["median_ms"]
        return dict(speedup_median=round(o["median_ms"] / c["median_ms"], 3), faster_margin_ms=round(faster, 3),
                    slower_margin_ms=round(slower, 3),
                    verdict="faster" if faster > 0 else "slower" if slower > 0 else "within spread")
    for name, (old, new) in parts.items():
        o, c = series(old), series(new)
        res[name] = dict(looped=o, many=c, ab=verdict(o, c))
    # the one kernel-side A/B: the pair order within a coarse launch
    ref = net.coarse_scores_many(pset, index, coarse=coarse)
    keep = gal_mod._coarse_pairs_order
    gal_mod._coarse_pairs_order = _entry_major
    try:
        alt = net.coarse_scores_many(pset, index, coarse=coarse)
        res["pair_order_same_bits"] = bool(torch.equal(bits(alt), bits(ref)))
        em = series(lambda: net.coarse_scores_many(pset, index, coarse=coarse))
    finally:
        gal_mod._coarse_pairs_order = keep
    pm = series(lambda: net.coarse_scores_many(pset, index, coarse=coarse))
    res["pair_order"] = dict(probe_major=pm, entry_major=em, ab=verdict(pm, em),
                             note="entry-major also scatters its scores back (one indexed copy per launch)")
    print("IDENTIFY_BENCH " + json.dumps(res), flush=True)


def child_subjects(args):
    """``--subjects R --shortlist M [--probes Q]``: the gallery labelled with R consecutive entries per
    subject.  On the Q x G coarse matrix of a probe set: ``ops.group_scores`` (max and mean) against
    ``ops.rank_select`` to M on the same matrix; then one probe's subject-level shortlisted query (both
    ``impressions``) against the entry-level one at the same M, in this one process."""
    import torch
    import bench
    import fpm
    from fpm import ops, params, synth
    dev = torch.device("cuda", 0)
    G, n, dtype, M, coarse, R = args.gallery, args.n, args.child, args.shortlist, args.coarse, args.subjects
    Q = args.probes or 16
    probes = [synth.make_graph(args.seed, p, 0, n) for p in range(Q)]
    base = bench.make_gallery(args.seed, 1, min(G, args.distinct), n, args.gen_workers)
    gallery = [base[i % len(base)] for i in range(G)]      # past --distinct graphs the gallery repeats them
    net = fpm.Net(regression=True, backbone=False, dtype=dtype)
    net.load_state_dict(params.init_params(args.seed))
    index = net.enroll(gallery, dev, subjects=[i // R for i in range(G)])
    pset = net.enroll(probes, dev)
    torch.cuda.synchronize()
    del gallery, base
    gt = index.subject_groups()
    S = int(gt["labels"].numel())
    res = dict(dtype=dtype, gallery=G, distinct_graphs=min(G, args.distinct), n=n, probes=Q, shortlist=M, per_subject=R,
               subjects=S, sc_mode=index.sc_mode, reps=args.reps, coarse=coarse)
    call = net.coarse_scores_many(pset, index, coarse=coarse)
    torch.cuda.synchronize()

    def series(fn):
        fn()
        torch.cuda.synchronize()
        return _ev(_timed(fn, args.reps))

    def fresh(fn):
        index._sel = None                  # every timed query stages its entries, as a new probe's would
        return fn()
    gs = torch.empty(Q, S, device=dev)
    gb = torch.empty(Q, S, device=dev, dtype=torch.int32)
    for fuse in ops.GROUP_FUSE:
        res["group_scores_%s" % fuse] = series(lambda: ops.group_scores(call, gt["off_d"], gt["pos_d"], fuse, gscore=gs,
                                                                         gbest=gb, off_host=gt["off"], pos_host=gt["pos"]))
    res["rank_select_entries"] = series(lambda: ops.rank_select(call, M))
    res["rank_select_subjects"] = series(lambda: ops.rank_select(gs, min(M, S)))
    res["matrix"] = "%d x %d" % (Q, G)
    probe = probes[0]
    res["entry_query"] = series(lambda: fresh(lambda: net.identify(probe, index, topk=10, shortlist=M, coarse=coarse)))
    for imp in ("all", "best"):
        q = lambda: net.identify(probe, index, topk=10, shortlist=M, coarse=coarse, by="subject", impressions=imp)
        res["subject_query_%s" % imp] = series(lambda: fresh(q))
        res["subject_query_%s" % imp]["exact_pairs"] = int(q()["short_idx"].numel())
    print("IDENTIFY_BENCH " + json.dumps(res), flush=True)


def _ab(o, c):
    """The project's A/B rule: the candidate's median against the baseline's best run less its spread."""
    faster = o["min_ms"] - (o["max_ms"] - o["min_ms"]) - c["median_ms"]
    slower = c["min_ms"] - (c["max_ms"] - c["min_ms"]) - o["median_ms"]
    return dict(speedup_median=round(o["median_ms"] / c["median_ms"], 3), faster_margin_ms=round(faster, 3),
                slower_margin_ms=round(slower, 3),
                verdict="faster" if faster > 0 else "slower" if slower > 0 else "within spread")


def child_prescreen(args):
    """``--shortlist M --prescreen K``: the prescreened query against the shortlisted query without it, in this one
    process; the prescreen's kernels alone; the coarse pass over K entries against the pass over the gallery."""
    import torch
    import bench
    import fpm
    from fpm import gallery as fgallery, ops, params, synth
    dev = torch.device("cuda", 0)
    G, n, dtype, M, K, coarse = args.gallery, args.n, args.child, args.shortlist, args.prescreen, args.coarse
    layout = args.layout
    probe = synth.make_graph(args.seed, 0, 0, n)
    base = bench.make_gallery(args.seed, 1, min(G, args.distinct), n, args.gen_workers)
    gal = [base[i % len(base)] for i in range(G)]          # past --distinct graphs the gallery repeats them
    net = fpm.Net(regression=True, backbone=False, dtype=dtype)
    net.load_state_dict(params.init_params(args.seed))
    index = net.enroll(gal, dev, layout=layout, descriptors=True)
    torch.cuda.synchronize()
    del gal, base
    res = dict(dtype=dtype, gallery=G, distinct_graphs=min(G, args.distinct), n=n, shortlist=M, prescreen=K,
               layout=layout, coarse=coarse, sc_mode=index.sc_mode, reps=args.reps, nbytes=index.nbytes(),
               desc_bytes=int(index.desc.numel()) * 2)

    def series(fn):
        fn()
        torch.cuda.synchronize()
        return _ev(_timed(fn, args.reps))

    def fresh(fn):
        index._sel = index._stage = None                   # a new probe's lists: nothing staged is kept
        return fn()
    pre = net.identify(probe, index, topk=10, shortlist=M, prescreen=K, coarse=coarse)
    plain = net.identify(probe, index, topk=10, shortlist=M, coarse=coarse)
    torch.cuda.synchronize()
    pre_idx = pre["pre_idx"].cpu().long()
    res["prescreen_kept"] = int(pre_idx.numel())
    res["plain_shortlist_in_prescreen"] = len(set(plain["short_idx"].tolist()) & set(pre_idx.tolist()))
    res["same_top1"] = int(plain["top_idx"][0]) == int(pre["top_idx"][0])
    wp = net.packed(dev)
    yp = net._probe_rows(wp, fgallery._ProbeSide(probe, index))
    one = torch.tensor([0, int(yp.shape[0])], dtype=torch.int64)
    one_d = one.to(dev)
    dq = ops.rows_pool(yp, one_d, row_off_host=one)
    sel = index.live
    sel32 = sel.to(torch.int32)
    sel_d = sel32.to(dev)
    sc = ops.desc_score(dq, index.desc, sel_d, idx_host=sel32)
    res["pool"] = series(lambda: ops.rows_pool(yp, one_d, out=dq, row_off_host=one))
    res["score"] = series(lambda: ops.desc_score(dq, index.desc, sel_d, out=sc, idx_host=sel32))
    res["score"]["desc_gb_per_s"] = round(res["desc_bytes"] / res["score"]["median_ms"] / 1e6, 1)
    res["keep"] = series(lambda: ops.rank_keep(sc, min(K, G)))
    res["prescreen_pass"] = series(lambda: (ops.rows_pool(yp, one_d, out=dq, row_off_host=one),
                                            fgallery._prescreen(dq, index, sel, K)))
    res["add_descriptors"] = series(lambda: index.add_descriptors())
    res["coarse_over_G"] = series(lambda: net.coarse_scores(probe, index, coarse=coarse))
    res["coarse_over_K"] = series(lambda: net.coarse_scores(probe, index, select=pre_idx, coarse=coarse))
    res["coarse_K_over_G"] = round(res["coarse_over_K"]["median_ms"] / res["coarse_over_G"]["median_ms"], 4)
    res["K_over_G"] = round(int(pre_idx.numel()) / G, 4)
    res["query"] = series(lambda: fresh(lambda: net.identify(probe, index, topk=10, shortlist=M, coarse=coarse)))
    res["query_prescreen"] = series(lambda: fresh(lambda: net.identify(probe, index, topk=10, shortlist=M, prescreen=K,
                                                                       coarse=coarse)))
    res["ab_coarse"] = _ab(res["coarse_over_G"], res["coarse_over_K"])
    res["ab_query"] = _ab(res["query"], res["query_prescreen"])
    res["planted"] = _planted_prescreen(dtype, layout)
    del index
    res["kernels_at_scale"] = _prescreen_kernels(series)
    print("IDENTIFY_BENCH " + json.dumps(res), flush=True)


def _prescreen_kernels(series):
    """The prescreen's kernels where the launch is not the cost: ``desc_score`` over 2^20 random unit descriptors
    (1.6 GB) for 1, 16 and 17 probes, ``rank_keep`` and ``rank_select`` over one row of 2^20 scores, ``rows_pool``
    over 8192 entries of 128 rows (3.2 GB)."""
    import torch
    from fpm import ops
    dev = torch.device("cuda", 0)
    out, G = {}, 1 << 20
    dg = torch.nn.functional.normalize(torch.randn(G, 768, device=dev), dim=1).to(torch.bfloat16)
    for Q in (1, 16, 17):
        dq, sc = dg[:Q].clone(), torch.empty(Q, G, device=dev)
        r = series(lambda: ops.desc_score(dq, dg, out=sc))
        r.update(probes=Q, entries=G, desc_tb_per_s=round(G * 1536 * ((Q + 15) // 16) / r["median_ms"] / 1e9, 3))
        out["score_Q%d" % Q] = r
    row = sc[:1].contiguous()
    for k in (1024, 65536):
        out["keep_k%d" % k] = dict(series(lambda: ops.rank_keep(row, k)), entries=G)
    out["select_k1024"] = dict(series(lambda: ops.rank_select(row, 1024)), entries=G)
    del dg, sc, row
    E, n = 8192, 128
    y = torch.randn(E * n, 768, device=dev)
    off = torch.arange(E + 1, dtype=torch.int64) * n
    off_d, d = off.to(dev), torch.empty(E, 768, device=dev, dtype=torch.bfloat16)
    r = series(lambda: ops.rows_pool(y, off_d, out=d, row_off_host=off))
    r.update(entries=E, rows_per_entry=n, rows_tb_per_s=round(int(y.numel()) * 4 / r["median_ms"] / 1e9, 3))
    out["pool"] = r
    return out


def _planted_prescreen(dtype, layout):
    """The tests' planted-mate gallery (40 entries, three probes, the "spread" weights): per probe the descriptor
    score of the mate and of the best other entry, and whether prescreen=8 keeps the mate."""
    import torch
    import fpm
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from test_shortlist_cpu import state_dicts
    from test_shortlist_gpu import MATES, planted
    dev = torch.device("cuda", 0)
    gal, probes = planted()
    net = fpm.Net(regression=True, backbone=False, dtype=dtype)
    net.load_state_dict(state_dicts()["spread"])
    index = net.enroll(gal, dev, batch=16, layout=layout, descriptors=True)
    out = []
    for p, r in enumerate(net.identify(probes, index, shortlist=4, prescreen=len(gal))):
        mate = [e for e, q in MATES.items() if q == p][0]
        sc = r["pre_score"].cpu()
        rest = torch.cat([sc[:mate], sc[mate + 1:]])
        kept = net.identify(probes[p], index, shortlist=4, prescreen=8)
        out.append(dict(mate_score=float(sc[mate]), best_other=float(rest.max()),
                        mate_kept_at_8=mate in kept["pre_idx"].tolist(), mate_first=int(kept["short_idx"][0]) == mate))
    return dict(gallery=len(gal), weights="spread", layout=layout, probes=out)


def main_prescreen(ap, args):
    """``--shortlist M --prescreen K``: one child per dtype over the ``--large`` gallery (``--gallery`` when 0)."""
    if "," in args.layout:
        ap.error("--prescreen takes one --layout")
    G, lines = args.large or args.gallery, []
    for dtype in args.dtypes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", dtype, "--gallery", str(G), "--n", str(args.n),
               "--reps", str(args.reps), "--seed", str(args.seed), "--gen-workers", str(args.gen_workers),
               "--shortlist", str(args.shortlist), "--prescreen", str(args.prescreen), "--distinct", str(args.distinct),
               "--coarse", args.coarse, "--layout", args.layout]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit("identify_bench: the %s x %d step ran over its %d s limit; stopping" % (dtype, G, args.step_timeout))
        got = [l for l in r.stdout.splitlines() if l.startswith("IDENTIFY_BENCH ")]
        if r.returncode != 0 or not got:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("identify_bench: the %s x %d step failed (exit %d); stopping" % (dtype, G, r.returncode))
        lines.append(json.loads(got[-1][len("IDENTIFY_BENCH "):]))
        print(json.dumps(lines[-1]), flush=True)
    out = args.out if args.out != ap.get_default("out") else os.path.join(REPO, "profiles", "identify_prescreen.json")
    doc = dict(tool="tools/identify_bench.py --shortlist %d --prescreen %d --layout %s --coarse %s --n %d"
                    % (args.shortlist, args.prescreen, args.layout, args.coarse, args.n),
               config="1 probe x gallery, n keypoints per graph, an index with descriptors; query = identify(shortlist=M) "
                      "(no prescreen: the parent side), query_prescreen = identify(shortlist=M, prescreen=K); pool, score "
                      "and keep: the prescreen's kernels alone, prescreen_pass: the three as the query runs them; "
                      "coarse_over_G / coarse_over_K: the coarse pass over the gallery and over the K kept entries; "
                      "weights are init_params: recall on trained weights is not measured",
               method="1 warm-up, `reps` queries each, HIP events around each query, median and min-max; both sides "
                      "in one process; a fresh process per shape",
               results=lines)
    if args.append and os.path.exists(out):
        with open(out) as f:
            old = json.load(f)
        doc["tool"] = old["tool"] + "; " + doc["tool"]
        doc["results"] = old["results"] + lines
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote %s" % out)


def main_shortlist(ap, args):
    lines = []
    shapes = [(args.gallery, dt) for dt in args.dtypes.split(",")]
    if args.large:
        shapes.append((args.large, args.dtypes.split(",")[0]))
    for G, dtype in shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", dtype, "--gallery", str(G), "--n", str(args.n),
               "--reps", str(args.reps), "--seed", str(args.seed), "--gen-workers", str(args.gen_workers),
               "--shortlist", str(args.shortlist), "--distinct", str(args.distinct), "--coarse", args.coarse,
               "--layout", args.layout, "--probes", str(args.probes), "--group-pairs", str(args.group_pairs),
               "--subjects", str(args.subjects)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit("identify_bench: the %s x %d step ran over its %d s limit; stopping" % (dtype, G, args.step_timeout))
        got = [l for l in r.stdout.splitlines() if l.startswith("IDENTIFY_BENCH ")]
        if r.returncode != 0 or not got:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("identify_bench: the %s x %d step failed (exit %d); stopping" % (dtype, G, r.returncode))
        lines.append(json.loads(got[-1][len("IDENTIFY_BENCH "):]))
        print(json.dumps(lines[-1]), flush=True)
    name = {"fused": "identify_shortlist.json", "wide": "identify_shortlist_wide.json",
            "auto": "identify_shortlist_wide.json"}.get(args.coarse, "identify_shortlist_stream.json")
    if args.layout != "f32":
        name = "identify_fp8.json" if "fp8+host" in args.layout.split(",") else "identify_compact.json"
    if args.probes:
        name = "identify_many.json"
    if args.subjects:
        name = "identify_subjects.json"
    out = args.out if args.out != ap.get_default("out") else os.path.join(REPO, "profiles", name)
    doc = dict(tool="tools/identify_bench.py%s --shortlist %d%s%s" % ((" --subjects %d" % args.subjects if args.subjects
                                                                       else "") +
                                                                      (" --probes %d" % args.probes if args.probes else ""),
                                                                      args.shortlist, "" if args.coarse == "fused" else
                                                                    " --coarse %s --n %d" % (args.coarse, args.n),
                                                                    "" if args.layout == "f32" else
                                                                    " --layout %s" % args.layout),
               config="gallery labelled with R consecutive entries per subject; group_scores (max, mean) and rank_select on "
                      "the same probes x gallery coarse matrix; one probe's subject-level shortlisted query (impressions "
                      "all / best) against the entry-level one at the same M" if args.subjects else
                      "1 probe x gallery, n keypoints per graph; full = identify over every entry (the path before "
                      "the shortlist existed), shortlisted = coarse pass + rank_select + identify over the M entries"
                      if not args.probes else
                      "%d probes x gallery, n keypoints per graph; looped = identify(list, shortlist=M), one probe at a "
                      "time; many = identify_many over the enrolled probe set; ms are per call, per_probe_ms per probe"
                      % args.probes,
               method="1 warm-up, `reps` queries each, HIP events around each query, median and min-max; both sides "
                      "in one process; a fresh process per shape",
               results=lines)
    if args.append and os.path.exists(out):
        with open(out) as f:
            old = json.load(f)
        doc["tool"] = old["tool"] + "; " + doc["tool"]
        doc["results"] = old["results"] + lines
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote %s" % out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shortlist", type=int, default=0,
                    help="M > 0: time identify(shortlist=M) against the full identify (profiles/identify_shortlist.json)")
    ap.add_argument("--coarse", choices=("fused", "wide", "auto", "stream", "any"), default="fused",
                    help="--shortlist: the coarse pass's kernel (wide / auto: profiles/identify_shortlist_wide.json; "
                         "stream / any: profiles/identify_shortlist_stream.json)")
    ap.add_argument("--layout", default="f32",
                    help="--shortlist: the index layout(s), comma-separated (f32, f32+bf16, bf16+host, fp8+host).  Anything but "
                         "the default 'f32' enrols the gallery once per layout in one process and records per layout "
                         "the bytes held, the coarse pass, the fetch, the M-pair forward and the whole shortlisted "
                         "query, the first layout the A/B baseline (profiles/identify_compact.json; with fp8+host, "
                         "which also records its coarse scores' shift against the baseline: profiles/identify_fp8.json)")
    ap.add_argument("--probes", type=int, default=0,
                    help="--shortlist: Q > 0 probes: the looped identify against identify_many "
                         "(profiles/identify_many.json)")
    ap.add_argument("--subjects", type=int, default=0,
                    help="--shortlist: R > 0 labels the gallery with R consecutive entries per subject and times "
                         "group_scores against rank_select on the --probes (default 16) x gallery coarse matrix, and the "
                         "subject-level shortlisted query against the entry-level one (profiles/identify_subjects.json)")
    ap.add_argument("--prescreen", type=int, default=0,
                    help="--shortlist: K > 0 times identify(shortlist=M, prescreen=K) against identify(shortlist=M) over "
                         "the --large gallery on one --layout (profiles/identify_prescreen.json)")
    ap.add_argument("--group-pairs", type=int, default=1024, help="--probes: identify_many's group_pairs")
    ap.add_argument("--append", action="store_true",
                    help="--shortlist: add the results to those the output file already holds (another --n)")
    ap.add_argument("--large", type=int, default=16384, help="--shortlist: a second, larger gallery (0: none)")
    ap.add_argument("--distinct", type=int, default=1024,
                    help="--shortlist: distinct graphs generated; a larger gallery repeats them (rows are enrolled apart)")
    ap.add_argument("--gallery", type=int, default=1024)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--gen-workers", type=int, default=8)
    ap.add_argument("--dtypes", default="bf16,f32")
    ap.add_argument("--step-timeout", type=int, default=240, help="time limit of one dtype's child, seconds")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "identify_c4.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if (args.probes or args.subjects or args.prescreen) and not args.shortlist > 0:
        ap.error("--probes, --subjects and --prescreen go with --shortlist M")
    if args.prescreen and (args.prescreen < args.shortlist or args.probes or args.subjects):
        ap.error("--prescreen K needs K >= --shortlist, without --probes and --subjects")
    if args.child:
        if args.prescreen:
            return child_prescreen(args)
        if args.subjects:
            return child_subjects(args)
        if args.probes:
            return child_probes(args)
        if args.shortlist > 0 and args.layout != "f32":
            return child_layouts(args)
        return child_shortlist(args) if args.shortlist > 0 else child(args)
    if args.prescreen:
        return main_prescreen(ap, args)
    if args.shortlist > 0:
        return main_shortlist(ap, args)
    lines = []
    for dtype in args.dtypes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", dtype, "--gallery", str(args.gallery), "--n",
               str(args.n), "--reps", str(args.reps), "--seed", str(args.seed), "--gen-workers", str(args.gen_workers)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit("identify_bench: the %s step ran over its %d s limit; stopping" % (dtype, args.step_timeout))
        got = [l for l in r.stdout.splitlines() if l.startswith("IDENTIFY_BENCH ")]
        if r.returncode != 0 or not got:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("identify_bench: the %s step failed (exit %d); stopping" % (dtype, r.returncode))
        lines.append(json.loads(got[-1][len("IDENTIFY_BENCH "):]))
        print(json.dumps(lines[-1]), flush=True)
    doc = dict(tool="tools/identify_bench.py", config="C4: 1 probe x gallery, n keypoints per graph",
               method="1 warm-up, median of `reps` forwards, HIP events around each forward; fresh process per dtype",
               results=lines)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()

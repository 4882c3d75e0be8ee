"""Benchmark: graph-match pairs/sec of the matcher's forward (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch 1024] [--n 256] [--dtype bf16]
                    [--dump-outputs DIR] [--full]

One step = one full ``Net.forward`` (eval, AFA-U regression, soft top-k, host Hungarian + greedy,
match classifier) over a batch of ``--batch`` synthetic pairs of ``--n``-keypoint Delaunay graphs
per GPU, inputs resident in HBM (graph generation is outside the timed region).  Multi-GPU:
launched by torch.distributed.run, one process per GPU, pairs sharded (no data-path collective;
gloo barrier + max-over-ranks timing only), ``value`` = pairs of all ranks / max rank time.
Rank 0 prints one JSON line.

A plain run sets up, warms up, times the K steps and prints the headline line.  ``--dump-outputs DIR``
also writes the last timed step's outputs as ``DIR/<name>.npy``.  ``--full`` adds everything else the
benchmark measures or checks after the timed steps: the profiled pass and roofline of the product
GEMM, the timed-batch self-check, the fp32 / 128-pair / strong-scaling lines, the on-device graph
build, the CPU-oracle baseline with the parity gate, and the c2 / c4 / c5 / training lines.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)


def _gen(args):
    seed, p, n = args
    from fpm import synth
    return (synth.make_graph(seed, p, 0, n), synth.make_graph(seed, p, 1, n))


def _under_profiler():
    """rocprofv3 preloads its tool library and initialises HSA before main: forked workers of such
    a process can hang, so graph generation stays in-process there."""
    return "rocprof" in os.environ.get("LD_PRELOAD", "") or any(k.startswith("ROCPROF") for k in os.environ)


def _gen_gallery(args):
    seed, g, n = args
    from fpm import synth
    return synth.make_graph(seed, g, 1, n)


def make_gallery(seed, first, G, n, workers):
    ids = [(seed, first + g, n) for g in range(G)]
    if workers <= 1 or G < 8 or _under_profiler():
        return [_gen_gallery(a) for a in ids]
    import multiprocessing as mp
    with mp.get_context("fork").Pool(workers) as pool:
        return pool.map(_gen_gallery, ids, chunksize=max(1, G // (workers * 4)))


def shard(config, rank, world, batch, gallery):
    """(first pair id, pairs on this rank).  c4: contiguous gallery shard (strong scaling, probe
    replicated); otherwise ``batch`` pairs per rank (weak scaling).  No data-path collective."""
    if config == "c4":
        share = (gallery + world - 1) // world
        first = min(rank * share, gallery)          # ranks past the end: empty shards at the end
        return first, max(0, min(share, gallery - first))
    return rank * batch, batch


def reduce_max(values, world):
    """Max over ranks of per-rank timings (gloo all_reduce; identity on one rank)."""
    if world <= 1:
        return list(values)
    import torch
    import torch.distributed as dist
    t = torch.tensor(values, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return t.tolist()


def make_pairs(seed, first, B, n, workers):
    ids = [(seed, first + b, n) for b in range(B)]
    if workers <= 1 or B < 8 or _under_profiler():
        return [_gen(a) for a in ids]
    import multiprocessing as mp
    with mp.get_context("fork").Pool(workers) as pool:
        return pool.map(_gen, ids, chunksize=max(1, B // (workers * 4)))


def cpu_baseline(n, npairs, seed, sd):
    """The CPU oracle (PyTorch CPU restatement of the same forward) on a bounded sample."""
    import torch
    import oracle as O
    # the box's CPU share (OMP_NUM_THREADS, 16 on the GPU pool), not the whole machine's affinity
    cores = max(1, min(int(os.environ.get("OMP_NUM_THREADS", "16")), len(os.sched_getaffinity(0))))
    torch.set_num_threads(cores)
    pairs = make_pairs(seed + 7919, 0, npairs, n, 1)
    O.forward(pairs[:1], sd)                   # warm-up
    t = time.perf_counter()
    ref = O.forward(pairs, sd)
    dt = time.perf_counter() - t
    return {"value": npairs / dt, "unit": "pairs/s", "cores": cores, "kind": "port",
            "sample": "%d pairs, n=%d, fp32 oracle forward incl. scipy Hungarian (1 process)" % (npairs, n)}, pairs, ref


def parity_vs_oracle(pairs, ref, sd, dev, dtypes):
    """The GPU forward (each compute mode) on the CPU baseline's own sample, against the oracle's
    outputs for it: max|d| per output and perm_mat agreement (SURVEY §8(d) parity gate: fp32 gated
    at 1e-4, bf16 reported).  Checker only: runs after the timed region."""
    import torch
    import fpm
    import oracle as O
    from fpm.batch import DeviceBatch
    out = {}
    for dt in dtypes:
        net = fpm.Net(regression=True, backbone=False, dtype=dt)
        net.load_state_dict(sd)
        res = net.run(DeviceBatch.from_pairs(pairs, dev))
        torch.cuda.synchronize()
        d = {k: float((res[k].float().cpu() - ref[k]).abs().max()) for k in ("ss", "ds_mat", "k_prob", "cls_prob")}
        P, R = res["perm_mat"].cpu(), ref["perm_mat"]
        d["perm_entries_agree"] = float((P == R).float().mean())
        d["perm_matches_kept"] = float((P * R).sum() / R.sum().clamp(min=1))
        d["perm_pairs_identical"] = float(np.mean([torch.equal(P[b], R[b]) for b in range(P.shape[0])]))
        # pair-by-pair class of every perm_mat difference (oracle.compare: select tie with the same
        # assignment, LSA near-tie whose assignment is optimal under the oracle's ds_mat within
        # m * 1e-6, eps-optimal assignment within 2 m delta (bf16 modes only), k* rounding crossing, or mismatch); every
        # differing pair carries its assignment gap under the oracle's ds_mat and the bound it met.
        # k* rounding crossings are judged against the mode's own k_prob bound (1e-4: the gate)
        gated = dt == "f32" or net.afau_mode == "bf16x3"
        rep = O.compare.perm_report(res, ref, [p[0]["n"] for p in pairs], [p[1]["n"] for p in pairs],
                                    reduced_precision=dt != "f32", k_tol=1e-4 if gated else 1.74e-3)
        d["perm_pairs_tie_equivalent"] = rep["tie_equivalent_frac"]
        d["afau_mode"] = net.afau_mode
        d["gate_1e-4_passed"] = all(d[k] < 1e-4 for k in ("ss", "ds_mat", "k_prob")) and rep["counts"]["mismatch"] == 0
        d["perm_classes"] = rep["counts"]
        d["perm_detail"] = {str(b): v for b, v in rep["detail"].items()}
        out[dt] = d
    out["pairs"] = len(pairs)
    return out


def timed_batch_selfcheck(net, bt, res):
    """The timed batch's own outputs against per-pair solo runs (the reference's forward loops
    pair by pair, ngm.py:326-361, so a pair's row must not depend on the batch around it): pair 0,
    the first pair of every pipeline chunk (incl. the halved tail chunks), the middle pair of the
    last chunk and the last pair, each re-run alone (one chunk, the batch's padded sizes) after the
    timed region and compared bit for bit with its row of the timed forward's outputs."""
    import torch
    K = net.pipeline_chunks(bt.B)
    parts = bt.split(K, net.tail_splits if K > 1 else 0)
    ranges = [p.pair_range if hasattr(p, "pair_range") else (0, bt.B) for p in parts]
    idx = sorted({0, bt.B - 1, (ranges[-1][0] + ranges[-1][1] - 1) // 2} | {r[0] for r in ranges})
    keys = ("s", "ss", "ds_mat", "perm_mat", "k_prob", "cls_prob")
    bad = []
    for b in idx:
        solo = net.run(bt.split_range(b, b + 1), chunks=1)
        for k in keys:
            if not torch.equal(solo[k][0], res[k][b]):
                bad.append((b, k))
    torch.cuda.synchronize()
    return {"identical": not bad, "pairs_checked": idx, "chunks": [list(r) for r in ranges],
            "outputs": list(keys), "mismatches": bad[:16]}


def bench_graph_build(kp, bt, dev, args):
    """On-device Delaunay graph build of both sides of the batch (fpm.graphs; untimed w.r.t. the
    metric: the reference builds graphs in DataLoader workers) vs scipy on a host sample; the
    device edge lists are checked against the host-built ones the bench ran on (full size)."""
    import torch
    from scipy.spatial import Delaunay
    from fpm import graphs
    P = [torch.from_numpy(k).to(dev) for k in kp]
    ns = [bt.n_host[0], bt.n_host[1]]
    for side in range(2):          # warm-up (module load)
        graphs.build_graph_batch(P[side][:4], ns[side][:4])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    gbs = [graphs.build_graph_batch(P[side], ns[side]) for side in range(2)]
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    mism = 0
    for side in range(2):
        g = gbs[side]
        if not (torch.equal(g.src, bt.src[side]) and torch.equal(g.dst, bt.dst[side])
                and torch.equal(g.pseudo, bt.pseudo[side])):
            mism += 1
    sample = min(64, kp[0].shape[0])
    t0 = time.perf_counter()
    for b in range(sample):
        Delaunay(kp[0][b].astype(np.float64))
    host = (time.perf_counter() - t0) / sample
    ngraph = 2 * kp[0].shape[0]
    return {"graphs": ngraph, "n": int(kp[0].shape[1]), "gpu_ms": e0.elapsed_time(e1), "wall_ms": wall * 1e3,
            "gpu_graphs_per_s": ngraph / (e0.elapsed_time(e1) / 1e3),
            "host_scipy_delaunay_ms_per_graph": host * 1e3,
            "edge_lists_identical_to_host": mism == 0}


def survey_flops_per_pair(n1, n2, E1, E2, d=768):
    """SURVEY §8(d)'s algorithmic FLOPs of one pair (the reference's per-edge SplineConv form, Ke
    excluded): 31.6 GFLOP at n = 256 (E = 1500), 15.3 at n = 128, 66.1 at n = 512."""
    N = n1 * n2
    f = 2 * (2 * (4 * E1 + n1) * d * d + 2 * (4 * E2 + n2) * d * d)               # SplineConv, 2 layers
    f += 2 * n1 * n2 * d + 4 * 1024 * d                                              # Kp
    f += sum((E1 * E2 + N) * C + N * (96 * C + 592) for C in (1, 17, 17))            # GNN layers
    f += 5 * 70 * N                                                                  # Sinkhorns
    f += 2 * (2 * 600 * 256 * (n1 + 2 * n2) + 2 * 16 * N * 16 * 2 + 16 * N * (130 + 5) + 2 * n1 * 256 * 600
              + 4 * n1 * 600 * 256 + 20 * n1 * 600)                                   # AFA-U
    f += 120 * N                                                                     # soft top-k
    f += 2 * (N * 144 + (N / 4) * 4608)                                              # MatchClassifier
    return float(f)


def exec_flops_per_pair(n1, n2, E1, E2, spline_rows, dtype, afau_mode="bf16x3", kp_x3=True, d=768):
    """FLOPs the device kernels EXECUTE per pair (the deduplicated (node, cell) product rows measured by
    fpm_profile_read, split-operand K where the bf16 mode runs near-fp32 products), by precision:
    -> ({stage: flops}, seconds per pair at the peaks of the precisions used).  bf16 MFMA stages are
    priced at 2.5 PF, everything else (fp32 MFMA / VALU) at 157.3 TF, so
    exec_frac = pairs/s x that time is the fraction of the step the kernels would need at peak (<= 1)."""
    N = n1 * n2
    bf = dtype == "bf16"
    x3 = bf and afau_mode == "bf16x3"
    f_bf, f_32 = {}, {}
    (f_bf if bf else f_32)["spline_product_gemm"] = 2.0 * spline_rows * d * d
    f_32["spline_combine"] = 2.0 * 2 * (2 * (4 * E1 + n1) * d + 2 * (4 * E2 + n2) * d)
    f_32["coef"] = 2.0 * 1024 * d
    (f_bf if bf else f_32)["vertex_affinity"] = 2.0 * N * d * (3 if (bf and kp_x3) else 1)
    f_32["gnn_layers"] = float(N * (640 + 2 * 2176) + (E1 * E2 + N) * (1 + 17 + 17))
    f_32["sinkhorns"] = 5.0 * 70 * N + 2 * 17 * N
    f_32["afau_attention"] = 16.0 * N * 99
    k = 3 if x3 else 1
    (f_bf if bf and afau_mode != "f32" else f_32)["afau_gemms"] = 2.0 * n1 * (256 * k * 600 + 640 * k * 256
                                                                              + 256 * k * 600)
    f_32["afau_norms"] = 2.0 * 20 * n1 * 600
    f_32["soft_topk"] = 120.0 * N
    f_32["match_classifier"] = 2.0 * (N * 144 + (N / 4) * 4608)
    t = sum(f_bf.values()) / 2.5e15 + sum(f_32.values()) / 157.3e12
    return {**f_bf, **f_32}, t, sum(f_bf.values()), sum(f_32.values())


def profiled_spline_rows(net, bt, pairs):
    """Product-GEMM rows per pair of one forward of ``bt`` (fpm_profile_read's FLOPs / 2 x 768^2)."""
    import ctypes
    import torch
    from fpm import _lib
    lib = _lib.load()
    lib.fpm_profile_read(None, None, None)
    lib.fpm_profile_enable(1)
    net.run(bt)
    torch.cuda.synchronize()
    lib.fpm_profile_enable(0)
    ms, fl, cnt = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    _lib.call("fpm_profile_read", ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(cnt))
    return fl.value / (2.0 * 768 * 768) / pairs


def spline_flops_per_graph(n, E, d=768):
    return float(2 * 2 * (4 * E + n) * d * d)


def config_line(cfg, args, dev, sd, steps=5, warmup=2):
    """One more SURVEY §8 config in the same run (N = 1): its pairs/s, its own parity gate against
    the fp32 oracle on a small sample, a bounded CPU-oracle baseline, and SURVEY §8(d)'s
    whole-forward roofline fraction.  c2: B = 256, n = 128, fp32; c4: 1 probe x 10 000 gallery graphs,
    n = 128, bf16, probe stage shared; c5: B = 1024, n = 512, bf16."""
    import torch
    import fpm
    import oracle as O
    from fpm import synth
    from fpm.batch import DeviceBatch
    n, B, dtype = {"c2": (128, 256, "f32"), "c4": (128, args.gallery, "bf16"), "c5": (512, 1024, "bf16")}[cfg]
    ncpu = {"c2": 8, "c4": 4, "c5": 2}[cfg]
    t0 = time.perf_counter()
    if cfg == "c4":
        probe = synth.make_graph(args.seed, 0, 0, n)
        gallery = make_gallery(args.seed, 1, B, n, args.gen_workers)
        bt = DeviceBatch.from_probe_gallery(probe, gallery, dev)
        sample = [(probe, g) for g in gallery[:ncpu]]
        E_pair = float(np.mean([g["edge_index"].shape[1] for g in gallery]))
        E_probe = float(probe["edge_index"].shape[1])
        del gallery
    else:
        pairs = make_pairs(args.seed, 0, B, n, args.gen_workers)
        bt = DeviceBatch.from_pairs(pairs, dev)
        E_pair = (bt.E[0] + bt.E[1]) / (2.0 * B)
        del pairs
        sample = make_pairs(args.seed + 7919, 0, ncpu, n, 1)
    gen_s = time.perf_counter() - t0
    net = fpm.Net(regression=True, backbone=False, dtype=dtype, lsa_threads=args.lsa_threads or None)
    net.load_state_dict(sd)
    for _ in range(warmup):
        net.run(bt)
    torch.cuda.synchronize()
    g_s = 0.0
    t0 = time.perf_counter()
    for _ in range(steps):
        net.run(bt)
        g_s += net.last_timing["gpu_stage_s"]
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    value = B * steps / el
    # SURVEY §8(d) accounting per pair; c4: each pair's gallery graph + pair stage, the shared
    # probe's SplineConv once per batch (the bench's stated accounting)
    if cfg == "c4":
        f_pair = (survey_flops_per_pair(n, n, E_probe, E_pair) - spline_flops_per_graph(n, E_probe)
                  + spline_flops_per_graph(n, E_probe) / B)
    else:
        f_pair = survey_flops_per_pair(n, n, E_pair, E_pair)
    peak = 2500.0 if dtype == "bf16" else 157.3
    rows = profiled_spline_rows(net, bt, B)
    if cfg == "c4":
        ex, t_ex, ex_bf, ex_32 = exec_flops_per_pair(n, n, 0, E_pair, rows, dtype, net.afau_mode, net.kp_x3)
    else:
        ex, t_ex, ex_bf, ex_32 = exec_flops_per_pair(n, n, E_pair, E_pair, rows, dtype, net.afau_mode, net.kp_x3)
    # the device on the CPU sample against the fp32 oracle: the gate (ss / ds_mat / k_prob 1e-4) and
    # perm classes with their recorded assignment gaps
    sbt = (DeviceBatch.from_probe_gallery(sample[0][0], [p[1] for p in sample], dev) if cfg == "c4"
           else DeviceBatch.from_pairs(sample, dev))
    res = net.run(sbt)
    torch.cuda.synchronize()
    cores = max(1, min(int(os.environ.get("OMP_NUM_THREADS", "16")), len(os.sched_getaffinity(0))))
    torch.set_num_threads(cores)
    t0 = time.perf_counter()
    ref = O.forward(sample, sd)
    cpu_dt = time.perf_counter() - t0
    d = {k: float((res[k].float().cpu() - ref[k]).abs().max()) for k in ("ss", "ds_mat", "k_prob", "cls_prob")}
    rep = O.compare.perm_report(res, ref, [p[0]["n"] for p in sample], [p[1]["n"] for p in sample],
                                reduced_precision=dtype != "f32", k_tol=1e-4)
    line = {"survey_config": cfg, "value": value, "unit": "pairs/s", "dtype": dtype, "steps": steps,
            "ms_per_step": el / steps * 1e3, "gpu_stage_pairs_per_s": B * steps / g_s if g_s > 0 else None,
            "pairs_per_step": B, "n_keypoints": n, "edges_per_graph": E_pair,
            "afau_mode": net.afau_mode,
            # hardware fraction: executed FLOPs at the peaks of the precisions they run in (<= 1)
            "exec_frac": value * t_ex, "exec_tflops": value * (ex_bf + ex_32) / 1e12,
            "exec_flops_per_pair": {"bf16_mfma": ex_bf, "fp32": ex_32, "spline_rows_per_pair": rows},
            # SURVEY §8(d)'s per-edge accounting: a rate in TFLOP/s, NOT a hardware fraction (the kernels
            # compute deduplicated (node, cell) rows, ~2.5x fewer FLOPs than the per-edge form)
            "rate_8d_tflops": value * f_pair / 1e12,
            "flops_per_pair_8d": f_pair, "peak_tflops": peak,
            "parity_gate": {"tolerance": 1e-4, "outputs": ["ss", "ds_mat", "k_prob"], "mode": dtype,
                            "passed": all(d[k] < 1e-4 for k in ("ss", "ds_mat", "k_prob"))
                            and rep["counts"]["mismatch"] == 0,
                            "max_abs": d, "perm_classes": rep["counts"],
                            "perm_detail": {str(b): v for b, v in rep["detail"].items()}, "pairs": len(sample)},
            "cpu_baseline": {"value": len(sample) / cpu_dt, "unit": "pairs/s", "cores": cores, "kind": "port",
                             "sample": "%d pairs, n=%d, fp32 oracle forward incl. scipy Hungarian" % (len(sample), n)},
            "input_gen_s": gen_s}
    if cfg == "c4":
        line["workload"] = "1 probe x %d gallery graphs, n=%d, probe SplineConv shared per pipeline chunk" % (B, n)
    del net, bt, sbt, res
    torch.cuda.empty_cache()
    return line


def train_line(args, dev, B=64, n=256, steps=4, warmup=2, cpu_pairs=2):
    """The training step in the driver's run: Net.forward in train mode +
    PermutationLoss + ks_loss + cls_loss, backward, AdamW (training_loop.py:23-70, stage 3's grouping
    with every parameter trainable) on B synthetic pairs, bf16; HIP-event split of the step; the CPU
    oracle's forward + autograd backward on a bounded sample beside it (tools/train_bench.py)."""
    import torch
    import fpm
    import oracle as O
    from fpm import params, synth, train
    from fpm.batch import DeviceBatch
    sd = params.init_params(1)
    pairs = synth.make_batch(3, B, n)
    bt = DeviceBatch.from_pairs(pairs, dev)
    gt = torch.zeros(B, n, n, device=dev)
    gt[:, torch.arange(n), torch.arange(n)] = 1.0
    label = (torch.arange(B, device=dev) % 2).float()
    net = fpm.Net(regression=True, backbone=False, dtype="bf16")
    net.load_state_dict(sd)
    net.to(dev).train()
    opt = torch.optim.AdamW([p for p in net.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-4)
    ns = [bt.n_host[0], bt.n_host[1]]

    def step(ev=None):
        opt.zero_grad(set_to_none=True)
        if ev:
            ev[0].record()
        out = net({"fpm_batch": bt, "gt_perm_mat": gt, "label": label})
        loss = train.permutation_loss(out["ds_mat"], gt, ns[0], ns[1]) + out["ks_loss"] + out["cls_loss"]
        if ev:
            ev[1].record()
        loss.backward()
        if ev:
            ev[2].record()
        opt.step()
        if ev:
            ev[3].record()
        return loss
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(steps)]
    t0 = time.perf_counter()
    for k in range(steps):
        loss = step(evs[k])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    res = {"metric": "training pairs/sec (forward + backward + AdamW)", "value": B / dt, "unit": "pairs/s",
           "ms_per_step": dt * 1e3, "forward_ms": sum(e[0].elapsed_time(e[1]) for e in evs) / steps,
           "backward_ms": sum(e[1].elapsed_time(e[2]) for e in evs) / steps,
           "optimizer_ms": sum(e[2].elapsed_time(e[3]) for e in evs) / steps,
           "batch": B, "n": n, "dtype": "bf16", "steps": steps, "loss_finite": bool(torch.isfinite(loss))}
    cores = max(1, min(int(os.environ.get("OMP_NUM_THREADS", "16")), len(os.sched_getaffinity(0))))
    torch.set_num_threads(cores)
    cp = pairs[:cpu_pairs]
    g = gt[:cpu_pairs].cpu()
    sdl = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running_" not in k else v.clone())
           for k, v in sd.items()}
    t = time.perf_counter()
    r = O.forward(cp, sdl, training=True, gt_perm=g, labels=label[:cpu_pairs].cpu())
    lo = O.permutation_loss(r["ds_mat"], g, [n] * len(cp), [n] * len(cp)) + r["ks_loss"] + r["cls_loss"]
    lo.backward()
    res["cpu_baseline"] = {"value": len(cp) / (time.perf_counter() - t), "unit": "pairs/s", "cores": cores,
                           "kind": "port", "sample": "%d pairs, n=%d, fp32 oracle forward + autograd backward"
                           % (len(cp), n)}
    del net, opt, bt
    torch.cuda.empty_cache()
    return res


def headline(args, world, net, pairs_total, elapsed, gpu_s, lsa_s, E_tot, tuning, shared_devices, cpu_share,
             pinned, t_gen, dumped):
    """The result line of a plain run (``--full`` adds its own fields to it): the timed steps' rate."""
    return {
        "metric": "graph-match pairs/sec @ n=256 kpts, batch=1024, 1 & 8 GPU",
        "value": pairs_total / elapsed,
        "unit": "pairs/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "strong" if args.config == "c4" else "weak",
        "vs_baseline": None,
        "dtype": args.dtype,
        "full": args.full,
        "data": "synthetic (seeded Delaunay keypoint graphs, random node/global features, random-init weights)",
        "config": {"workload": ("1 probe x %d gallery graphs (%d per GPU), n=%d keypoints, probe SplineConv "
                                "once per pipeline chunk (accounting: shared probe stage), %s MFMA; full "
                                "Net.forward per pair" % (args.gallery, args.batch, args.n, args.dtype))
                   if args.config == "c4" else
                   ("batch=%d pairs/GPU, n=%d keypoints, Delaunay edges, factorized Kronecker "
                    "affinity, %s MFMA; full Net.forward incl. AFA-U, soft top-k, host Hungarian, "
                    "greedy top-k, MatchClassifier" % (args.batch, args.n, args.dtype)),
                   "survey_config": args.config,
                   "afau_mode": net.afau_mode,
                   "global_batch": args.gallery if args.config == "c4" else args.batch * world,
                   "n_keypoints": args.n,
                   "edges_per_graph": E_tot / (2.0 * args.batch), "parallelism": "pair-sharded x%d" % world},
        "gpu_stage_pairs_per_s": args.batch * world * args.steps / gpu_s,
        "host_lsa_ms_per_step": lsa_s / args.steps * 1e3,
        "tuning": tuning or None,
        "ranks_share_devices": shared_devices,
        "host_cpus_per_rank": cpu_share,
        "ranks_pinned": pinned is not None,
        "input_gen_s": t_gen,
        "dumped_outputs": dumped,
    }


DUMP_BYTES = 48 << 20     # budget of one --dump-outputs directory (limit: 64 MB)


def dump_outputs(res, out_dir, seed=0):
    """Write the arrays of one forward's result dict as ``out_dir/<name>.npy`` (float32; integer and
    float64 outputs as float64).  Outputs too large for their share of DUMP_BYTES are cut to a fixed,
    seeded sample of whole pairs (their indices: ``sample_pairs.npy``), or of flat elements where one
    pair alone is too large.  -> {name: shape written}."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    arrs = {k: v for k, v in res.items() if torch.is_tensor(v)}
    share = DUMP_BYTES // max(1, sum(v.numel() * 4 > (1 << 20) for v in arrs.values()))
    rng = np.random.default_rng(seed)
    written, pick = {}, {}
    for k in sorted(arrs):
        v = arrs[k].detach()
        if v.numel() * 4 > max(share, 1 << 20):
            row = (v.numel() // v.shape[0]) * 4
            if v.dim() >= 2 and row <= share:
                B = v.shape[0]
                if B not in pick:
                    pick[B] = np.sort(rng.choice(B, max(1, min(B, share // row)), replace=False))
                v = v[torch.from_numpy(pick[B]).to(v.device)]
            else:
                idx = np.sort(rng.choice(v.numel(), share // 4, replace=False))
                v = v.reshape(-1)[torch.from_numpy(idx).to(v.device)]
        a = v.cpu()
        a = (a.double() if a.dtype in (torch.float64, torch.int64, torch.int32) else a.float()).numpy()
        np.save(os.path.join(out_dir, k + ".npy"), a)
        written[k] = list(a.shape)
    for B, idx in pick.items():
        np.save(os.path.join(out_dir, "sample_pairs.npy" if len(pick) == 1 else "sample_pairs_%d.npy" % B),
                idx.astype(np.float64))
    return written


def log(*a):
    print("[bench %.1fs]" % (time.perf_counter() - T0), *a, file=sys.stderr, flush=True)


T0 = time.perf_counter()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024, help="pairs per GPU")
    ap.add_argument("--n", type=int, default=256, help="keypoints per graph")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps, write the last "
                    "timed step's outputs as DIR/<name>.npy (large ones: a fixed, seeded sample of pairs)")
    ap.add_argument("--full", action="store_true", help="after the timed steps also run everything else the "
                    "benchmark measures or checks (profiled pass / roofline, self-check, fp32 / share / strong "
                    "lines, graph build, CPU baseline + parity gate, c2 / c4 / c5 / training lines); the "
                    "--no-* switches and --cpu-pairs / --parity-pairs select among these")
    ap.add_argument("--cpu-pairs", type=int, default=32)
    ap.add_argument("--parity-pairs", type=int, default=32, help="pairs of the CPU sample re-run on the GPU "
                    "modes for the parity_vs_oracle report (and the parity_gate)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-f32-line", action="store_true", help="skip the fp32-mode C3 line")
    ap.add_argument("--no-share-line", action="store_true", help="skip the 128-pairs-per-GPU line")
    ap.add_argument("--no-selfcheck", action="store_true", help="skip the timed-batch self-check (kernel-trace "
                    "profiles: its single-pair forwards would enter the per-kernel averages)")
    ap.add_argument("--no-config-lines", action="store_true", help="skip the c2 / c4 / c5 / training lines of the "
                    "default run")
    ap.add_argument("--lsa-threads", type=int, default=0)
    ap.add_argument("--gen-workers", type=int, default=16)
    ap.add_argument("--config", default="c3", choices=["c2", "c3", "c4", "c5"],
                    help="SURVEY §8 configs: c3 = the headline (n=256, 1024 pairs/GPU, bf16); c2 = n=128, "
                         "256 pairs/GPU, fp32; c4 = 1 probe x --gallery graphs (n=128) sharded over ranks, probe "
                         "stage shared; c5 = n=512, 1024 pairs/GPU")
    ap.add_argument("--gallery", type=int, default=10000, help="c4: gallery size over all ranks")
    ap.add_argument("--tuning", default="", help="kernel-variant switches for A/B runs, key=value[,key=value] "
                    "(fpm_set_tuning keys, include/fpm.h); recorded in the JSON line")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.config == "c2":
        args.n, args.batch, args.dtype = 128, 256, "f32"
    elif args.config == "c5":
        args.n = 512
    elif args.config == "c4":
        args.n = 128

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher: start one rank per GPU as children (nothing has touched the GPU yet) and
        # exit with their status, so --gpus N never silently measures one GPU
        import subprocess
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(29500 + os.getpid() % 1000),
               os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    if world != args.gpus:
        raise SystemExit("bench: WORLD_SIZE=%d but --gpus=%d" % (world, args.gpus))
    # stdout carries exactly one JSON line: anything native code writes to fd 1 (gloo prints
    # "[Gloo] Rank r is connected to ..." from every rank at rendezvous) goes to stderr instead
    json_out = os.fdopen(os.dup(1), "w")
    sys.stdout.flush()
    os.dup2(2, 1)

    # inputs first (forked workers must not inherit a GPU context)
    t_gen = time.perf_counter()
    first, args.batch = shard(args.config, rank, world, args.batch, args.gallery)
    if args.config == "c4":
        # contiguous gallery shard per rank; the probe is replicated
        g0 = first
        from fpm import synth
        probe = synth.make_graph(args.seed, 0, 0, args.n)
        gallery = make_gallery(args.seed, 1 + g0, args.batch, args.n, args.gen_workers)
        pairs = None
    else:
        pairs = make_pairs(args.seed, first, args.batch, args.n, args.gen_workers)
    t_gen = time.perf_counter() - t_gen
    log("generated %d pairs in %.1fs" % (args.batch, t_gen))

    import torch
    import torch.distributed as dist
    import fpm
    from fpm import _lib, params
    from fpm.batch import DeviceBatch

    if world > 1:
        dist.init_process_group("gloo")
    # several ranks on the node: each rank's host Hungarian pool on its own slice of the CPUs
    from fpm.model import pin_rank_cpus, host_cpu_share
    pinned = pin_rank_cpus()
    if pinned is not None:
        log("rank %d pinned to %d CPUs (%d..%d)" % (rank, len(pinned), pinned[0], pinned[-1]))
    # one GPU per rank; with fewer visible GPUs than ranks (a rehearsal of the N-rank path on a
    # smaller box) ranks share devices round-robin and say so in the JSON
    ndev = torch.cuda.device_count()
    shared_devices = ndev < world
    torch.cuda.set_device(local % ndev)
    dev = torch.device("cuda", local % ndev)
    tuning = {}
    for kv in filter(None, args.tuning.split(",")):
        key, val = kv.split("=")
        from fpm import ops as _ops
        _ops.set_tuning(key, int(val))
        tuning[key] = int(val)
    sd = params.init_params(args.seed)
    net = fpm.Net(regression=True, backbone=False, dtype=args.dtype, lsa_threads=args.lsa_threads or None)
    net.load_state_dict(sd)
    if args.config == "c4":
        bt = DeviceBatch.from_probe_gallery(probe, gallery, dev)
        del gallery
    else:
        bt = DeviceBatch.from_pairs(pairs, dev)
        kp = [np.stack([p[side]["P"] for p in pairs]).astype(np.float32) for side in range(2)]
        del pairs
    E_tot = bt.E[0] + bt.E[1]

    def barrier():
        if world > 1:
            dist.barrier()

    log("batch on device, E/graph=%.1f" % (E_tot / (2.0 * args.batch)))
    for _ in range(args.warmup):
        net.run(bt)
        log("warmup step: gpu-stage %.3fs lsa %.3fs" % (net.last_timing["gpu_stage_s"], net.last_timing["lsa_s"]))
    torch.cuda.synchronize()
    # the torch streams the forward uses (their pool index fixes the HIP stream, hence the hardware queue)
    log("streams: " + " ".join("%s=%d" % (k, v.stream_id) for k, v in net._stream_cache.items()
                                 if hasattr(v, "stream_id")) + " compute=" +
        ",".join(str(st.stream_id) for st in net._streams(dev)))
    lib = _lib.load()
    import ctypes

    last = {}       # each timed loop's final outputs (kept for the self-check after the timing)

    def timed(model, batch, steps, tag):
        """``steps`` forwards bracketed by barrier + synchronize -> (wall s, gpu-stage s, lsa s)."""
        g_s = l_s = 0.0
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            last[tag] = model.run(batch)
            lt = model.last_timing
            g_s += lt["gpu_stage_s"]
            l_s += lt["lsa_s"]
            log("%s step: gpu-stage %.3fs lsa %.3fs enqueue %.3fs first-chunk %.3fs total %.3fs" % (
                tag, lt["gpu_stage_s"], lt["lsa_s"], lt["enqueue_s"], lt["first_chunk_wait_s"], lt["total_s"]))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        barrier()
        return t1 - t0, g_s, l_s

    # the headline: K steps with the library's profiling off
    elapsed, gpu_s, lsa_s = timed(net, bt, args.steps, "")
    dumped = None
    if args.dump_outputs:
        # what the last timed step returned (each rank its own shard's, rank r > 0 under rank<r>/)
        dumped = dump_outputs(last[""], os.path.join(args.dump_outputs, "rank%d" % rank) if rank
                              else args.dump_outputs, args.seed)
        log("outputs written to %s: %s" % (args.dump_outputs, json.dumps(dumped)))
    pairs_total = (args.gallery if args.config == "c4" else args.batch * world) * args.steps
    if not args.full:
        # a plain run: the headline line only
        del last[""]
        elapsed, gpu_s, lsa_s = reduce_max([elapsed, gpu_s, lsa_s], world)
        if rank == 0:
            res = headline(args, world, net, pairs_total, elapsed, gpu_s, lsa_s, E_tot, tuning, shared_devices,
                           host_cpu_share(), pinned, t_gen, dumped)
            print(json.dumps(res), file=json_out, flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    # the roofline: the same K steps again, every product-GEMM launch bracketed by HIP events on its
    # own stream (fpm_profile_*); its wall rate is reported beside the headline
    lib.fpm_profile_read(None, None, None)     # drop earlier records
    lib.fpm_profile_enable(1)
    elapsed_prof, _, _ = timed(net, bt, args.steps, "profiled")
    lib.fpm_profile_enable(0)
    ms = ctypes.c_double()
    fl = ctypes.c_double()
    cnt = ctypes.c_int()
    _lib.call("fpm_profile_read", ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(cnt))
    # the same kernel without the second stream's kernels sharing the CUs (one extra, untimed
    # forward on one stream): its isolated rate, reported beside the in-pipeline one
    iso_ms = ctypes.c_double()
    iso_fl = ctypes.c_double()
    iso_cnt = ctypes.c_int()
    saved_streams = net.n_streams
    net.n_streams = 1
    lib.fpm_profile_enable(1)
    net.run(bt)
    torch.cuda.synchronize()
    lib.fpm_profile_enable(0)
    net.n_streams = saved_streams
    _lib.call("fpm_profile_read", ctypes.byref(iso_ms), ctypes.byref(iso_fl), ctypes.byref(iso_cnt))
    # the timed batch's rows against per-pair solo runs (after every timing of this rank)
    selfcheck = ({"identical": None, "pairs_checked": [], "chunks": [], "outputs": []} if args.no_selfcheck
                 else timed_batch_selfcheck(net, bt, last[""]))
    log("timed-batch self-check: %s" % json.dumps(selfcheck))
    if selfcheck["identical"] is False:
        raise SystemExit("bench: timed batch differs from per-pair solo runs: %s" % selfcheck["mismatches"])
    del last[""]
    elapsed, gpu_s, lsa_s, elapsed_prof = reduce_max([elapsed, gpu_s, lsa_s, elapsed_prof], world)
    value = pairs_total / elapsed
    peak = 2500.0 if args.dtype == "bf16" else 157.3
    achieved = (fl.value / (ms.value / 1e3)) / 1e12 if ms.value > 0 else 0.0
    # executed FLOPs per pair from the profiled steps' product rows (bench.exec_flops_per_pair)
    rows_pp = fl.value / (2.0 * 768 * 768) / max(pairs_total / world, 1)
    Eg = E_tot / (2.0 * args.batch)
    ex_f, ex_t, ex_bf, ex_32 = exec_flops_per_pair(args.n, args.n, 0 if args.config == "c4" else Eg, Eg, rows_pp,
                                                   args.dtype, net.afau_mode, net.kp_x3)

    # the fp32 (parity) mode on the same C3 batch beside the bf16 headline
    f32_line = None
    if args.dtype == "bf16" and args.config == "c3" and not args.no_f32_line:
        net32 = fpm.Net(regression=True, backbone=False, dtype="f32", lsa_threads=args.lsa_threads or None)
        net32.load_state_dict(sd)
        net32.run(bt)
        k32 = max(1, min(args.steps, 3))
        e32, g32, _ = timed(net32, bt, k32, "f32")
        e32, g32 = reduce_max([e32, g32], world)
        _, t32, b32, s32 = exec_flops_per_pair(args.n, args.n, Eg, Eg, rows_pp, "f32", "f32", False)
        v32 = args.batch * world * k32 / e32
        f32_line = {"value": v32, "unit": "pairs/s", "dtype": "f32", "steps": k32,
                    "ms_per_step": e32 / k32 * 1e3, "gpu_stage_pairs_per_s": args.batch * world * k32 / g32,
                    "exec_frac": v32 / world * t32, "exec_tflops": v32 * (b32 + s32) / 1e12}
        del net32
        torch.cuda.empty_cache()

    # strong scaling: BASELINE's global batch (args.batch pairs) split over the ranks; each rank runs
    # the first batch/world pairs of its own shard (same graph-size distribution)
    strong = None
    if world > 1 and args.config != "c4":
        share = max(1, args.batch // world)
        sub = bt.split_range(0, share)
        net.run(sub)
        es, gs_, _ = timed(net, sub, args.steps, "strong")
        es, gs_ = reduce_max([es, gs_], world)
        strong = {"global_batch": share * world, "pairs_per_gpu": share, "value": share * world * args.steps / es,
                  "unit": "pairs/s", "ms_per_step": es / args.steps * 1e3, "scaling": "strong"}

    # the strong-scaling share on one GPU: BASELINE's global batch of 1024 over 8 GPUs is 128 pairs
    # per GPU; the same forward timed on the first 128 pairs of this batch (its own line, not value)
    share_line = None
    if world == 1 and args.config == "c3" and args.batch >= 256 and not args.no_share_line:
        sub = bt.split_range(0, 128)
        net.run(sub)
        es, gs_, ls_ = timed(net, sub, args.steps, "share128")
        share_line = {"pairs_per_gpu": 128, "value": 128 * args.steps / es, "unit": "pairs/s",
                      "ms_per_step": es / args.steps * 1e3, "gpu_stage_pairs_per_s": 128 * args.steps / gs_,
                      "host_lsa_ms_per_step": ls_ / args.steps * 1e3, "chunks": net.last_timing["chunks"],
                      "enqueue_ms": net.last_timing["enqueue_s"] * 1e3,
                      "note": "BASELINE's global batch of 1024 split over 8 GPUs: 128 pairs per GPU, one GPU timed"}
        log("share-128 line: %s" % json.dumps(share_line))

    # HBM bytes per launch of the same kernel from the committed rocprofv3 PMC pass (FETCH_SIZE x2 +
    # WRITE_SIZE, separate passes; tools/pmc_gemm.sh -> profiles/r01_pmc_product_gemm.json)
    traffic = None
    pdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    pmc_name = next((f for f in ("r06_pmc_product_gemm.json", "r05zz2_pmc_product_gemm.json", "r05z2_pmc_product_gemm.json", "r04v_pmc_product_gemm.json", "r04_pmc_product_gemm.json", "r03_pmc_product_gemm.json", "r02_pmc_product_gemm.json",
                                         "r01_pmc_product_gemm.json")
                     if os.path.exists(os.path.join(pdir, f))), None)
    if args.dtype == "bf16" and args.config == "c3" and pmc_name:
        with open(os.path.join(pdir, pmc_name)) as f:
            traffic = json.load(f).get("traffic_bytes_per_launch")

    graph_build = None
    if rank == 0 and args.config != "c4":
        graph_build = bench_graph_build(kp, bt, dev, args)
        log("graph build: %s" % json.dumps(graph_build))

    if rank == 0:
        cpu = parity = None
        if world == 1 and not args.no_cpu_baseline:
            log("cpu baseline ...")
            cpu, cpu_pairs, cpu_ref = cpu_baseline(args.n, args.cpu_pairs, args.seed, sd)
            log("cpu baseline %.3f pairs/s" % cpu["value"])
            if args.config != "c4":
                # the GPU modes on the baseline's own sample against the oracle's outputs for it
                parity = parity_vs_oracle(cpu_pairs[:args.parity_pairs], {k: v[:args.parity_pairs] for k, v in
                                                                          cpu_ref.items() if torch.is_tensor(v)
                                                                          and v.dim() >= 1 and v.shape[0] == len(cpu_pairs)},
                                          sd, dev, ["bf16", "f32"] if args.dtype == "bf16" else [args.dtype])
                log("parity vs oracle: %s" % json.dumps(parity))
        # the other SURVEY §8 configs in the driver's own run (N = 1, after everything above)
        config_lines = {}
        if world == 1 and args.config == "c3" and not args.no_config_lines:
            del bt
            torch.cuda.empty_cache()
            for cfg in ("c2", "c4", "c5"):
                config_lines[cfg + "_line"] = config_line(cfg, args, dev, sd)
                log("%s line: %s" % (cfg, json.dumps(config_lines[cfg + "_line"])))
            config_lines["train_line"] = train_line(args, dev)
            log("train line: %s" % json.dumps(config_lines["train_line"]))
        f8d = survey_flops_per_pair(args.n, args.n, E_tot / (2.0 * args.batch), E_tot / (2.0 * args.batch))

        res = headline(args, world, net, pairs_total, elapsed, gpu_s, lsa_s, E_tot, tuning, shared_devices,
                       host_cpu_share(), pinned, t_gen, dumped)
        res.update({
            "roofline": {"kernel": "spline (node, cell) product GEMM (%s, grouped by cell)" % (("gemm_phase_kernel 256x256" if os.environ.get("FPM_GEMM_PHASE", "1") != "0" else "gemm_big_kernel<256>") if args.dtype == "bf16" else "gemm_kernel<f32>"),
                         "bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
                         "frac": achieved / peak, "traffic": traffic,
                         "traffic_unit": "HBM bytes per launch (rocprofv3 PMC, profiles/%s)" % pmc_name,
                         "traffic_source": "the committed PMC pass of the same kernel and config (separate FETCH_SIZE / "
                                           "WRITE_SIZE runs, tools/pmc_gemm.sh); not measured in this run",
                         "duration_note": "achieved / avg_launch_ms: HIP events around each launch on its stream in "
                                          "the two-stream pipeline, so they include the co-running kernels' share of "
                                          "the CUs; isolated_*: one extra single-stream forward",
                         "launches": cnt.value, "avg_launch_ms": ms.value / max(cnt.value, 1),
                         "algorithmic_flops_per_launch": fl.value / max(cnt.value, 1),
                         "isolated_achieved": (iso_fl.value / (iso_ms.value / 1e3)) / 1e12 if iso_ms.value > 0 else 0.0,
                         "isolated_avg_launch_ms": iso_ms.value / max(iso_cnt.value, 1),
                         # the whole forward's hardware fraction: executed FLOPs (deduplicated product
                         # rows from this run's profile, split-operand K) at the peaks of the precisions
                         # they run in (bench.exec_flops_per_pair), <= 1
                         "exec_frac": value / world * ex_t, "exec_tflops": value * (ex_bf + ex_32) / 1e12,
                         "exec_flops_per_pair": {"bf16_mfma": ex_bf, "fp32": ex_32, "spline_rows_per_pair": rows_pp,
                                                 "by_stage": ex_f},
                         # SURVEY §8(d)'s per-edge accounting as a rate (TFLOP/s): NOT a hardware
                         # fraction (the reference's per-edge form, ~2.5x the executed FLOPs)
                         "rate_8d_tflops": None if args.config == "c4" else value * f8d / 1e12,
                         "flops_per_pair_8d": None if args.config == "c4" else f8d},
            "value_profiled": pairs_total / elapsed_prof,
            "cpu_baseline": cpu,
            "parity_vs_oracle": parity,
            # north-star gate on the headline mode itself: ss / ds_mat / k_prob within 1e-4 of the fp32
            # CPU oracle on the baseline's sample, every perm_mat pair identical or explained
            "parity_gate": None if not parity or args.dtype not in parity else {
                "tolerance": 1e-4, "outputs": ["ss", "ds_mat", "k_prob"], "mode": args.dtype,
                "afau_mode": parity[args.dtype]["afau_mode"], "passed": parity[args.dtype]["gate_1e-4_passed"],
                "max_abs": {k: parity[args.dtype][k] for k in ("ss", "ds_mat", "k_prob", "cls_prob")},
                "perm_classes": parity[args.dtype]["perm_classes"],
                "perm_detail": parity[args.dtype]["perm_detail"], "pairs": parity["pairs"]},
            "timed_batch_selfcheck": selfcheck["identical"],
            "timed_batch_selfcheck_detail": {k: selfcheck[k] for k in ("pairs_checked", "chunks", "outputs")},
            "f32_line": f32_line,
            "strong_scaling": strong,
            "share128_line": share_line,
            "graph_build": graph_build,
        })
        res.update(config_lines)
        print(json.dumps(res), file=json_out, flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

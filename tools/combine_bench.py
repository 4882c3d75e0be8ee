"""Time one SplineConv side-layer (product GEMM + combine) on bench-shaped inputs per tuning
variant, run under rocprofv3 --kernel-trace; with ``--parse DIR`` print each variant's per-kernel
mean durations from the trace (variants run in order, REPS layers each).

    rocprofv3 --kernel-trace -d gpurun_out/cb -o run --output-format csv -- python tools/combine_bench.py combine_lds_kb=0 combine_lds_kb=40
    python tools/combine_bench.py --parse gpurun_out/cb combine_lds_kb=0 combine_lds_kb=40
"""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS = int(os.environ.get("REPS", 10))


def variants(argv):
    return [tuple((k, int(v)) for k, v in (kv.split("=") for kv in a.split(","))) for a in argv] or [()]


def parse(d, vs):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    for name in ("combine_kernel", "gemm_walk_kernel"):
        ks = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if name in r["Kernel_Name"]]
        ks = ks[len(ks) - len(vs) * (REPS + 1):]           # the last (REPS + 1) per variant
        for i, v in enumerate(vs):
            seg = ks[i * (REPS + 1) + 1:(i + 1) * (REPS + 1)]     # first of each variant = warm-up
            seg = sorted(seg)
            print("%-18s %-40s median %.4f ms  min %.4f ms" % (name, v, seg[len(seg) // 2] / 1e6, seg[0] / 1e6))


def main():
    if sys.argv[1:2] == ["--parse"]:
        return parse(sys.argv[2], variants(sys.argv[3:]))
    import torch
    import fpm
    from fpm import ops, params, synth
    from fpm.batch import DeviceBatch
    dev = torch.device("cuda", 0)
    B, n = 128, 256
    bt = DeviceBatch.from_pairs(synth.make_batch(3, B, n), dev)
    net = fpm.Net(regression=True, backbone=False, dtype="bf16")
    net.load_state_dict(params.init_params(1))
    wp = net.packed(dev)
    side = 0
    nn_ = B * n
    plan = ops.spline_plan(bt.src[side], bt.dst[side], bt.pseudo[side], nn_, n, bt.max_graph_edges(side))
    x_op = ops.cast_bf16(bt.x[side])
    yws = ops.spline_y_ws(ops.BF16, bt.E[side], nn_, dev)
    out = torch.empty(nn_, 768, device=dev, dtype=torch.bfloat16)
    for var in variants(sys.argv[1:]):
        prev = [(k, ops.set_tuning(k, v)) for k, v in var]
        for _ in range(REPS + 1):
            ops.spline_conv(x_op, plan, bt.E[side], nn_, n, bt.n[side], wp["W0"], wp["bias0"], yws, 0, out_t=out)
        torch.cuda.synchronize()
        for k, v in prev:
            ops.set_tuning(k, v)


if __name__ == "__main__":
    main()

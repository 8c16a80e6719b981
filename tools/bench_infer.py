#!/usr/bin/env python
"""The batch-tiled inference kernel (csrc/mlp_infer.hip) against mlp_eval_kernel, on one GPU, in one process.

  models  5-64-2 and 5-128-128-2            rows  20,000 and 1,000,000
  outputs statistics only (loss sum + correct count; the new kernel also its confusion matrix), and logits + statistics

Every configuration is built and warmed first; then ROUNDS rounds, each timing every configuration once (alternating,
so drift hits all alike): a host clock around CALLS launches that end in a device synchronise.  Reported per
configuration: the median and the min .. max of the rounds, us per launch, and rows per second at the median.  Both
kernels read the same table through the same index list (a permutation) and the same parameters; a launch of the old
kernel includes zeroing its two accumulators, a launch of the new one its fold launch.  The tool fails without a GPU;
it sets no threshold.

    python tools/bench_infer.py [--rounds 9] [--label TEXT] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODELS = ([5, 64, 2], [5, 128, 128, 2])
ROWS = (20000, 1000000)


def configs(dims, n, dev):
    import torch

    from dct_amd.ops.fused_mlp import FusedMLPKernel, mlp_num_params

    g = torch.Generator().manual_seed(0)
    p = ((torch.rand(mlp_num_params(dims), generator=g) * 2 - 1) * 0.3).to(dev)
    X = torch.randn(n, dims[0], generator=g).to(dev)
    Y = torch.randint(0, dims[-1], (n,), generator=g, dtype=torch.int32).to(dev)
    idx = torch.randperm(n, generator=g).to(torch.int32).to(dev)
    kern = FusedMLPKernel(dims, bmax=1024)
    acc = torch.zeros(2, device=dev)
    stats = torch.zeros(2 + dims[-1] ** 2, dtype=torch.int64, device=dev)
    logits = torch.empty(n, dims[-1], device=dev)
    name = "-".join(map(str, dims)) + " n=%d " % n
    out = []
    for what, lo in (("stats", None), ("logits+stats", logits)):
        def old(lo=lo):
            acc.zero_()
            kern.evaluate(p, X, Y, idx, n, acc, logits_out=lo)

        def new(lo=lo):
            kern.infer(p, X, n, idx=idx, Y=Y, logits_out=lo, stats_out=stats)

        out.append((name + what + ": mlp_eval_kernel", old, n))
        out.append((name + what + ": mlp_infer", new, n))
    # the two kernels agree on what they count (the run is no benchmark of a wrong answer)
    old()
    new()
    torch.cuda.synchronize()
    loss_sum, correct, _ = kern.infer_stats(stats)
    a = acc.tolist()
    if int(a[1]) != correct and n < 2 ** 24:
        raise SystemExit("bench_infer: correct counts differ: %r vs %d" % (a[1], correct))
    if abs(a[0] - loss_sum) > 1e-3 * abs(loss_sum):
        raise SystemExit("bench_infer: loss sums differ: %r vs %r" % (a[0], loss_sum))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--label", default="", help="printed with the results (which tree this is)")
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    import torch

    import dct_amd  # noqa: F401

    if not torch.cuda.is_available():
        raise SystemExit("bench_infer.py needs a GPU")
    dev = torch.device("cuda", 0)
    built = []
    for dims in MODELS:
        for n in ROWS:
            for name, run, rows in configs(dims, n, dev):
                calls = 2000 if n <= 20000 else 200
                for _ in range(3):  # warm-up: code objects, the workspace, every shape of the timed window
                    run()
                torch.cuda.synchronize()
                built.append((name, run, rows, calls))
    times = {name: [] for name, _, _, _ in built}
    for _ in range(a.rounds):
        for name, run, _, calls in built:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / calls * 1e6)
    lines = ["bench_infer %s: %s, %d alternating rounds, us per launch (median, min .. max), rows/s at the median"
             % (a.label, torch.cuda.get_device_name(0), a.rounds)]
    out = {}
    for name, _, rows, calls in built:
        t = times[name]
        med = statistics.median(t)
        lines.append("  %-56s %10.2f  (%.2f .. %.2f)  %.3e rows/s  [%d launches per round]"
                     % (name, med, min(t), max(t), rows / med * 1e6, calls))
        out[name] = {"median_us": med, "min_us": min(t), "max_us": max(t)}
    lines.append(json.dumps({"label": a.label, "rounds": a.rounds, "us_per_launch": out}))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

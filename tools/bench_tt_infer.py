#!/usr/bin/env python
"""The whole-model TabTransformer inference kernel (csrc/tt_infer.hip) against the path it replaces, on one GPU, in
one process.

  model   4 blocks (64 features, d_model 64, 4 heads, FFN 256), 2 classes      rows  20,000 and 200,000
  outputs statistics only (loss sum + correct count; the new kernel also its confusion matrix), and logits + statistics

The replaced path is what Trainer.validate ran for this model: ``model.eval()``, ``torch.no_grad()``, batches of 512
through ``model(x)`` (one tt_block launch per block, torch's pooling, LayerNorm and bf16 head) plus the loss and
accuracy ops of ``validation_step``, their sums kept on the device.  The new path is one ``tt_infer`` call: packing the
two parameter images, the kernel and its fold launch.

Every configuration is built and warmed first; then ROUNDS rounds, each timing every configuration once (alternating,
so drift hits all alike): a host clock around CALLS calls that end in a device synchronise.  Reported per
configuration: the median and the min .. max of the rounds, ms per call, rows per second and - from the blocks'
FLOPs, 7.34 MFLOP per block and sample - the achieved TFLOP/s at the median; then new / old.  The tool fails without
a GPU; it sets no threshold.

    python tools/bench_tt_infer.py [--rounds 9] [--label TEXT] [--out FILE]
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

LAYERS, CLASSES, BATCH = 4, 2, 512
ROWS = (20000, 200000)
# QKV, projection, FC1, FC2 over 64 tokens, and S = Q K^T, P V of 4 heads of 16
BLOCK_FLOP = 2 * 64 * (64 * 192 + 64 * 64 + 64 * 256 + 256 * 64) + 4 * 2 * 2 * 64 * 64 * 16


def configs(model, n, dev):
    import torch
    import torch.nn.functional as F

    from dct_amd.ops.nn import tt_infer

    g = torch.Generator().manual_seed(0)
    X = torch.randn(n, 64, generator=g).to(dev)
    Y = torch.randint(0, CLASSES, (n,), generator=g)
    Y32, Y64 = Y.to(dev, torch.int32), Y.to(dev)
    stats = torch.zeros(2 + CLASSES ** 2, dtype=torch.int64, device=dev)
    logits = torch.empty(n, CLASSES, device=dev)
    acc = torch.zeros(2, dtype=torch.float64, device=dev)
    out = []
    for what, lo in (("stats", None), ("logits+stats", logits)):
        @torch.no_grad()
        def old(lo=lo):
            acc.zero_()
            for b in range(0, n, BATCH):
                y = Y64[b: b + BATCH]
                z = model(X[b: b + BATCH])
                acc[0] += F.cross_entropy(z, y, reduction="sum")
                acc[1] += (z.argmax(1) == y).sum()
                if lo is not None:
                    lo[b: b + BATCH] = z

        def new(lo=lo):
            tt_infer(model, X, n, Y=Y32, logits_out=lo, stats_out=stats)

        out.append(("n=%d %s: model(x) in batches of %d" % (n, what, BATCH), old, n))
        out.append(("n=%d %s: tt_infer" % (n, what), new, n))
    # the two paths agree on what they count (the run is no benchmark of a wrong answer)
    old()
    new()
    host, a = stats.cpu(), acc.tolist()
    loss_sum, correct = float(host[:1].view(torch.float64)[0]), int(host[1])
    if abs(a[1] - correct) > 0.01 * n or abs(a[0] - loss_sum) > 1e-2 * abs(loss_sum):
        raise SystemExit("bench_tt_infer: the paths differ: loss %r vs %r, correct %r vs %d" % (a[0], loss_sum, a[1], correct))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--label", default="", help="printed with the results (which tree this is)")
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    import torch

    import dct_amd  # noqa: F401
    from dct_amd.models.tabtransformer import TabTransformer

    if not torch.cuda.is_available():
        raise SystemExit("bench_tt_infer.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = TabTransformer(layers=LAYERS, num_classes=CLASSES).to(dev).eval()
    built = []
    for n in ROWS:
        for name, run, rows in configs(model, n, dev):
            for _ in range(2):  # warm-up: code objects, the workspace, every shape of the timed window
                run()
            torch.cuda.synchronize()
            built.append((name, run, rows, 5 if n <= 20000 else 2))
    times = {name: [] for name, _, _, _ in built}
    for _ in range(a.rounds):
        for name, run, _, calls in built:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / calls * 1e3)
    lines = ["bench_tt_infer %s: %s, %d alternating rounds, ms per call (median, min .. max), rows/s and block TFLOP/s "
             "at the median" % (a.label, torch.cuda.get_device_name(0), a.rounds)]
    out = {}
    for name, _, rows, calls in built:
        t = times[name]
        med = statistics.median(t)
        lines.append("  %-48s %9.3f  (%.3f .. %.3f)  %.3e rows/s  %7.2f TFLOP/s  [%d calls per round]"
                     % (name, med, min(t), max(t), rows / med * 1e3, rows * LAYERS * BLOCK_FLOP / med * 1e-9, calls))
        out[name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t)}
    for (old, _, _, _), (new, _, _, _) in zip(built[0::2], built[1::2]):
        lines.append("  %-48s new / old = %.3f" % (new, out[new]["median_ms"] / out[old]["median_ms"]))
    lines.append(json.dumps({"label": a.label, "rounds": a.rounds, "ms_per_call": out}))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
